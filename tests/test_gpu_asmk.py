"""GPU tests of the ASMK* index (csrc/asmk.hip, pvsim.ASMKIndex): both kernels and the index against the NumPy twin
(tests/asmk_numpy.py), bit for bit -- include/pvsim.h defines every sum, and the score is a sum of integers, so there is no
tolerance to argue about."""
import numpy as np
import pytest

import asmk_numpy as tw

pytestmark = pytest.mark.gpu

F = np.float32
DESC_F32, DESC_U8_ROOTSIFT = 0, 2
FILL = 0x5A


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a) if a.nbytes else ctx.buffer(16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------------------------ aggregate
def _lattice(rng, K, D, levels=4):
    """K distinct centroids with coordinates in 4 * {0 .. levels - 1}"""
    seen = set()
    while len(seen) < K:
        seen.add(tuple((rng.randint(0, levels, D) * 4).tolist()))
    return np.array(sorted(seen), F)


def _near(rng, cent, words):
    """rows on the lattice around their centroid: coordinates moved by -1, 0 or +1"""
    words = np.asarray(words, np.int64)
    return (cent[words] + rng.randint(-1, 2, (len(words), cent.shape[1]))).astype(F)


def _edge_images(rng, cent, big=300):
    K = len(cent)
    images = [np.zeros((0, cent.shape[1]), F),                            # no rows
              _near(rng, cent, [K - 1]),                                  # one row
              _near(rng, cent, [3 % K] * 70),                             # all rows on one word (more than a wave of rows)
              _near(rng, cent, rng.permutation(K)),                       # every row on a different word
              cent[[1 % K]].copy(),                                       # a row exactly on its centroid
              _near(rng, cent, rng.randint(0, K, big)),
              np.zeros((0, cent.shape[1]), F),
              _near(rng, cent, rng.randint(0, K, 65))]
    images[5][7] = cent[rng.randint(0, K)]                                # ... and one inside a longer image
    return images


def _aggregate(ctx, rows_list, cent, kind, proj, bits):
    """pvs_kmeans_predict_dev + pvs_asmk_aggregate_dev on a batch -> (labels, words, sigs, counts), the slot arrays as they are"""
    D, W = cent.shape[1], bits // 32
    dt = np.uint8 if kind == DESC_U8_ROOTSIFT else F
    off = np.zeros(len(rows_list) + 1, np.int64)
    np.cumsum([len(r) for r in rows_list], out=off[1:])
    total, n = int(off[-1]), len(rows_list)
    packed = np.concatenate(rows_list).astype(dt) if total else np.zeros((0, D), dt)
    cb = ctx.codebook(cent)
    bufs = [_up(ctx, packed), _up(ctx, off), ctx.buffer(max(total, 4) * 4), ctx.buffer(max(total, 4) * 4).fill_bytes(FILL),
            ctx.buffer(max(total, 4) * 4 * W).fill_bytes(FILL), ctx.buffer(n * 4).fill_bytes(FILL)]
    d_x, d_off, d_lab, d_word, d_sig, d_cnt = bufs
    d_p = _up(ctx, proj) if proj is not None else None
    try:
        if total:
            ctx.kmeans_predict_dev(cb, d_x.ptr, kind, total, d_lab.ptr)
        ctx.asmk_aggregate_dev(cb, d_x.ptr, kind, d_off.ptr, off, n, total, d_lab.ptr, d_p.ptr if d_p else None, bits, d_word.ptr,
                               d_sig.ptr, d_cnt.ptr)
        out = (d_lab.download((total,), np.int32), d_word.download((total,), np.int32), d_sig.download((total, W), np.uint32),
               d_cnt.download((n,), np.int32), off)
    finally:
        cb.close()
        for b in bufs + ([d_p] if d_p else []):
            b.free()
    return out


def _check_aggregate(got, values_list, cent, proj):
    """values_list: the float32 value of every row as the header defines it (RootSIFT applied).  Asserts the gap of the inputs, the
    labels, every entry, the counts, and that the slots beyond count[i] still hold the fill pattern."""
    labels, words, sigs, counts, off = got
    fill32 = np.uint32(int.from_bytes(bytes([FILL] * 4), "little"))
    for i, x in enumerate(values_list):
        lo, hi = int(off[i]), int(off[i + 1])
        want_lab, gap = tw.labels_and_gap(x, cent)
        assert gap > 1e-3, f"image {i}: the test's own rows are too close to a decision boundary ({gap})"
        assert np.array_equal(labels[lo:hi], want_lab), f"image {i}: labels"
        w, s = tw.image_entries(x, want_lab, cent, proj)
        assert counts[i] == len(w), f"image {i}: {counts[i]} entries, the twin has {len(w)}"
        assert np.array_equal(words[lo:lo + len(w)], w), f"image {i}: words"
        assert np.array_equal(sigs[lo:lo + len(w)], s), f"image {i}: signatures"
        assert (words[lo + len(w):hi].view(np.uint32) == fill32).all() and (sigs[lo + len(w):hi] == fill32).all(), f"image {i}: slots past the count"


@pytest.mark.parametrize("D,B,with_p", [(32, 32, False), (128, 128, False), (128, 64, True), (20, 32, True), (2, 32, True)])
def test_aggregate_matches_twin(gpu_ctx, D, B, with_p):
    rng = np.random.RandomState(1700 + D + B)
    K = 16 if D == 2 else 40
    cent = _lattice(rng, K, D)
    proj = rng.standard_normal((B, D)).astype(F) if with_p else None
    images = _edge_images(rng, cent)
    got = _aggregate(gpu_ctx, images, cent, DESC_F32, proj, B)
    _check_aggregate(got, images, cent, proj)
    on_centroid = got[2][int(got[4][4])]                                  # image 4: one row on its centroid -> all ones
    assert (on_centroid == 0xFFFFFFFF).all()
    assert got[3].tolist()[:5] == [0, 1, 1, K, 1]


def test_aggregate_image_of_8192_rows_and_the_refusal(gpu_ctx):
    rng = np.random.RandomState(1760)
    cent = _lattice(rng, 64, 32, levels=2)
    images = [_near(rng, cent, rng.randint(0, 64, 8192)), _near(rng, cent, rng.randint(0, 64, 5))]
    _check_aggregate(_aggregate(gpu_ctx, images, cent, DESC_F32, None, 32), images, cent, None)
    images[1] = _near(rng, cent, rng.randint(0, 64, 8193))
    with pytest.raises(NotImplementedError, match="8193"):
        _aggregate(gpu_ctx, images, cent, DESC_F32, None, 32)


def test_aggregate_with_65536_words(gpu_ctx):
    """centroid w has the 16 bits of w in its first 16 coordinates (times 4): word 65535 is in use"""
    rng = np.random.RandomState(1770)
    w = np.arange(65536)
    cent = np.zeros((65536, 32), F)
    cent[:, :16] = ((w[:, None] >> np.arange(16)[None, :]) & 1) * 4
    images = [_near(rng, cent, [65535, 0, 65535, 40000, 65534, 1]), _near(rng, cent, rng.randint(0, 65536, 40)), _near(rng, cent, [65535])]
    got = _aggregate(gpu_ctx, images, cent, DESC_F32, None, 32)
    _check_aggregate(got, images, cent, None)
    assert got[1][int(got[4][0]) + got[3][0] - 1] == 65535


def test_aggregate_u8_rootsift(gpu_ctx):
    """uint8 raw SIFT rows at D = 128: the values are the twin's float32 sqrt(raw / (sum + 1e-7)); centroids are RootSIFT rows of
    prototypes, rows are prototypes moved by a few counts"""
    rng = np.random.RandomState(1780)
    K = 24
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)
    proto[0, :] = 0
    proto[0, 3] = 255                                                      # a one-bin row
    cent = tw.rootsift(proto)

    def rows(words):
        return np.clip(proto[words].astype(np.int64) + rng.randint(-2, 3, (len(words), 128)), 0, 255).astype(np.uint8)

    images = [rows(rng.randint(0, K, 150)), np.zeros((0, 128), np.uint8), rows([5]), proto[[7, 7, 0]].copy(), rows(rng.permutation(K))]
    got = _aggregate(gpu_ctx, images, cent, DESC_U8_ROOTSIFT, None, 128)
    _check_aggregate(got, [tw.rootsift(r) for r in images], cent, None)
    proj = rng.standard_normal((96, 128)).astype(F)
    got = _aggregate(gpu_ctx, images, cent, DESC_U8_ROOTSIFT, proj, 96)
    _check_aggregate(got, [tw.rootsift(r) for r in images], cent, proj)


def test_aggregate_refuses_bad_arguments(gpu_ctx):
    rng = np.random.RandomState(1790)
    cent = _lattice(rng, 8, 32)
    images = [_near(rng, cent, [1, 2])]
    with pytest.raises(ValueError):
        _aggregate(gpu_ctx, images, cent, DESC_F32, None, 64)             # no projection: bits must equal D
    with pytest.raises(ValueError):
        _aggregate(gpu_ctx, images, cent, DESC_F32, np.zeros((48, 32), F), 48)


# ------------------------------------------------------------------------------------------------ score
def _entries(rng, n, K, W, lo=0, hi=10, flips=None):
    """n images of lo..hi random words.  flips = None: random signatures (Hamming distances around B / 2, where sel is zero);
    otherwise the signature of word w is one base pattern per word with up to `flips` random bits flipped, so that two images
    that share a word are close"""
    base = rng.randint(0, 1 << 32, (K, W), dtype=np.uint64).astype(np.uint32)
    out = []
    for _ in range(n):
        words = np.sort(rng.permutation(K)[:rng.randint(lo, hi + 1)]).astype(np.int32)
        if flips is None:
            out.append((words, rng.randint(0, 1 << 32, (len(words), W), dtype=np.uint64).astype(np.uint32)))
        else:
            out.append(_near_sigs(rng, (words, base[words]), flips))
    return out


def _near_sigs(rng, ent, flips=6):
    """the same words with a few bits flipped: Hamming distances where sel is not zero"""
    words, sigs = ent
    s = sigs.copy()
    for e in range(len(words)):
        for _ in range(rng.randint(0, flips + 1)):
            s[e, rng.randint(0, s.shape[1])] ^= np.uint32(1) << np.uint32(rng.randint(0, 32))
    return words.copy(), s


def _flat(ents, W):
    off = np.zeros(len(ents) + 1, np.int64)
    np.cumsum([len(e[0]) for e in ents], out=off[1:])
    words = np.concatenate([e[0] for e in ents]).astype(np.int32) if ents else np.zeros(0, np.int32)
    sigs = np.concatenate([e[1].reshape(-1, W) for e in ents]).astype(np.uint32) if ents else np.zeros((0, W), np.uint32)
    return off, words, sigs


class _Db:
    """the inverted file of a list of entries, resident"""

    def __init__(self, ctx, db, K, bits, wt, sel):
        self.ctx, self.K, self.bits, self.N = ctx, K, bits, len(db)
        word_off, ent_img, ent_sig = tw.invert(db, K)
        gdb = np.array([tw.gamma(x[0], wt) for x in db], F)
        self.host = (word_off, ent_img, ent_sig, gdb)
        self.bufs = [_up(ctx, a) for a in (word_off, ent_img, ent_sig.reshape(-1, bits // 32), gdb, np.asarray(wt, np.int32),
                                           np.asarray(sel, np.int32))]

    def score(self, queries, wt, slice_images=0, ld=None):
        W = self.bits // 32
        off, words, sigs = _flat(queries, W)
        gq = np.array([tw.gamma(q[0], wt) for q in queries], F)
        nq, ld = len(queries), self.N if ld is None else ld
        d_w, d_s, d_g = _up(self.ctx, words), _up(self.ctx, sigs), _up(self.ctx, gq)
        d_out = self.ctx.buffer(max(nq * ld, 4) * 4).fill_bytes(FILL)
        b = self.bufs
        try:
            self.ctx.asmk_score_dev(nq, off, d_w.ptr, d_s.ptr, self.bits, self.K, b[0].ptr, b[1].ptr, b[2].ptr, self.N, b[4].ptr, b[5].ptr,
                                    d_g.ptr, b[3].ptr, d_out.ptr, ld, slice_images)
            return d_out.download((nq, ld), F)
        finally:
            for x in (d_w, d_s, d_g, d_out):
                x.free()

    def close(self):
        for b in self.bufs:
            b.free()


def test_score_slices_and_seams(gpu_ctx):
    """N = 200 in slices of 64 (seams at 64, 128, 192), of 128 and of the host's choice: identical bits, equal to the twin's pair
    loop.  Word 5 is held by the images 63, 64, 127, 128 and 199 alone."""
    rng = np.random.RandomState(1800)
    K, bits, N = 30, 128, 200
    db = _entries(rng, N, K, 4, lo=1, hi=10, flips=24)
    for i, (words, sigs) in enumerate(db):
        keep = words != 5
        db[i] = (words[keep], sigs[keep])
    for i in (63, 64, 127, 128, 199):
        words = np.append(db[i][0], 5).astype(np.int32)
        order = np.argsort(words)
        db[i] = (words[order], np.concatenate([db[i][1], rng.randint(0, 1 << 32, (1, 4), dtype=np.uint64).astype(np.uint32)])[order])
    wt, sel = tw.word_weights(db, K), tw.selectivity(bits, 3.0, 0.0)
    word_off, ent_img, _ = tw.invert(db, K)
    assert ent_img[word_off[5]:word_off[6]].tolist() == [63, 64, 127, 128, 199]
    queries = [_near_sigs(rng, db[i]) for i in (63, 64, 128, 199, 0)] + _entries(rng, 2, K, 4, lo=3)
    want = tw.scores(queries, db, wt, sel)
    assert (want > 0).sum() > N and np.unique(want).size > 50
    d = _Db(gpu_ctx, db, K, bits, wt, sel)
    try:
        base = d.score(queries, wt, 0)
        assert np.array_equal(_bits(base), _bits(want))
        for s in (64, 128, 256):
            assert np.array_equal(_bits(d.score(queries, wt, s)), _bits(base)), f"slice_images = {s}"
        for bad in (32, 100, 32768 + 64, -64):
            with pytest.raises(ValueError):
                d.score(queries, wt, bad)
    finally:
        d.close()


def test_score_long_list_inside_one_slice(gpu_ctx):
    """every image holds word 0: a list of 700 entries (more than 512: the whole wave walks it in eleven steps) inside the single
    slice the host chooses for N = 700; slices of 64 cut the same list into eleven parts, which lane groups walk side by side"""
    rng = np.random.RandomState(1810)
    K, bits, N = 3, 32, 700
    db = []
    for _ in range(N):
        words = np.array([0] + ([2] if rng.randint(0, 2) else []), np.int32)
        db.append((words, rng.randint(0, 1 << 8, (len(words), 1), dtype=np.uint64).astype(np.uint32)))      # close signatures
    wt, sel = np.array([7, 0, 300], np.int32), tw.selectivity(bits, 1.0, 0.0)
    assert tw.invert(db, K)[0][1] == 700
    queries = [db[0], db[699], (np.array([0], np.int32), np.array([[0]], np.uint32)), (np.array([2], np.int32), np.array([[255]], np.uint32))]
    want = tw.scores(queries, db, wt, sel)
    d = _Db(gpu_ctx, db, K, bits, wt, sel)
    try:
        assert np.array_equal(_bits(d.score(queries, wt, 0)), _bits(want))
        assert np.array_equal(_bits(d.score(queries, wt, 64)), _bits(want))
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64, 96, 128])
def test_score_edge_entries_and_padding(gpu_ctx, bits):
    """a query with no entries, an image with no entries, a query word whose list is empty (only the query holds it), ld > N with
    the padding left untouched; three queries in one call equal three calls of one"""
    rng = np.random.RandomState(1820 + bits)
    K, W, N = 20, bits // 32, 70
    db = _entries(rng, N, K - 1, W, lo=1, hi=8, flips=bits // 6)           # word K - 1 is held by no image
    db[11] = (np.zeros(0, np.int32), np.zeros((0, W), np.uint32))
    wt, sel = tw.word_weights(db, K), tw.selectivity(bits, 3.0, 0.2)
    assert wt[K - 1] == 0
    lonely = (np.array([K - 1], np.int32), np.ones((1, W), np.uint32))
    with_lonely = (np.append(db[4][0], K - 1).astype(np.int32), np.concatenate([db[4][1], np.ones((1, W), np.uint32)]))
    queries = [_near_sigs(rng, db[3], 4), (np.zeros(0, np.int32), np.zeros((0, W), np.uint32)), lonely, with_lonely, _near_sigs(rng, db[69], 3)]
    want = tw.scores(queries, db, wt, sel)
    assert (_bits(want[1]) == 0).all() and (_bits(want[2]) == 0).all() and (_bits(want[:, 11]) == 0).all() and want[3, 4] > 0.99
    d = _Db(gpu_ctx, db, K, bits, wt, sel)
    try:
        got = d.score(queries, wt, 0, ld=N + 5)
        assert np.array_equal(_bits(got[:, :N]), _bits(want))
        assert (got[:, N:].view(np.uint8) == FILL).all()
        assert np.array_equal(_bits(d.score(queries, wt, 64)), _bits(want))
        for q in range(3):
            assert np.array_equal(_bits(d.score(queries[q:q + 1], wt, 0)), _bits(want[q:q + 1]))
    finally:
        d.close()


def test_score_conversion_rounds_beyond_2_to_24(gpu_ctx):
    """17 shared identical entries at wt = sel[0] = 1023: acc = 17 * 1023 * 1023 = 17790993 is odd and above 2^24, so the
    conversion to float32 must round (to nearest even)"""
    K, bits, W = 40, 64, 2
    rng = np.random.RandomState(1830)
    words = np.arange(3, 20, dtype=np.int32)
    sigs = rng.randint(0, 1 << 32, (17, W), dtype=np.uint64).astype(np.uint32)
    db = [(words, sigs), (words[:5], sigs[:5]), (np.arange(25, 40, dtype=np.int32), rng.randint(0, 1 << 32, (15, W), dtype=np.uint64).astype(np.uint32))]
    wt, sel = np.full(K, 1023, np.int32), tw.selectivity(bits, 3.0, 0.0)
    acc = tw.pair_acc(db[0], db[0], wt, sel)
    assert acc == 17 * 1023 * 1023 and acc > 1 << 24 and int(F(np.uint32(acc))) != acc
    want = tw.scores(db[:1], db, wt, sel)
    d = _Db(gpu_ctx, db, K, bits, wt, sel)
    try:
        assert np.array_equal(_bits(d.score(db[:1], wt, 0)), _bits(want))
    finally:
        d.close()


def test_score_more_queries_than_one_launch_holds(gpu_ctx):
    """130 queries: the entry offsets of a launch travel as kernel arguments, 128 queries at a time"""
    rng = np.random.RandomState(1840)
    K, bits, N = 12, 32, 40
    db = _entries(rng, N, K, 1, lo=1, hi=5, flips=6)
    wt, sel = tw.word_weights(db, K), tw.selectivity(bits, 3.0, 0.0)
    queries = [_near_sigs(rng, db[rng.randint(0, N)], 3) for _ in range(130)]
    want = tw.scores(queries, db, wt, sel)
    d = _Db(gpu_ctx, db, K, bits, wt, sel)
    try:
        assert np.array_equal(_bits(d.score(queries, wt, 0)), _bits(want))
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tiny(gpu_ctx):
    """a dozen tiny images of uint8 rows around 30 prototypes, and their float32 RootSIFT values"""
    from pvsim.verify import LocalFeatureIndex
    rng = np.random.RandomState(1850)
    K = 30
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)
    cent = tw.rootsift(proto)

    def rows(words):
        return np.clip(proto[words].astype(np.int64) + rng.randint(-2, 3, (len(words), 128)), 0, 255).astype(np.uint8)

    sizes = [0, 1, 7, 25, 40, 3, 12, 30, 18, 9, 22, 5]
    images = [rows(rng.randint(0, K, n)) for n in sizes]
    queries = [images[4][::2].copy(), np.concatenate([images[7][:15], rows(rng.randint(0, K, 6))]), np.zeros((0, 128), np.uint8)]
    local = LocalFeatureIndex.from_arrays(images, [np.zeros((len(r), 6), F) for r in images], [f"im{i}" for i in range(12)], ctx=gpu_ctx)
    yield cent, images, queries, local
    local.close()


@pytest.mark.parametrize("bits,projection", [(128, None), (64, "random")])
def test_index_equals_the_twin(gpu_ctx, tiny, bits, projection, tmp_path):
    from pvsim import ASMKIndex
    cent, images, queries, local = tiny
    values = [tw.rootsift(r) for r in images]
    for x in values + [tw.rootsift(q) for q in queries]:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3
    proj = tw.random_projection(bits, 128, 9) if projection else None
    db = tw.entries(values, cent, proj)
    K = len(cent)
    wt, sel = tw.word_weights(db, K), tw.selectivity(bits, 3.0, 0.0)
    word_off, ent_img, ent_sig = tw.invert(db, K)
    index = ASMKIndex.build(local, cent, bits=bits, projection=projection, random_state=9)
    try:
        assert len(index) == 12 and index.paths == [f"im{i}" for i in range(12)]
        if proj is not None:
            assert np.array_equal(index.projection, proj)
        assert np.array_equal(index.word_off, word_off) and np.array_equal(index.ent_img, ent_img)
        assert np.array_equal(index.ent_sig, ent_sig) and np.array_equal(index.list_sizes(), np.diff(word_off))
        assert np.array_equal(index.wt, wt) and np.array_equal(index.sel, sel)
        assert np.array_equal(_bits(index.gamma_db), _bits(np.array([tw.gamma(x[0], wt) for x in db], F)))
        want = tw.scores(tw.entries([tw.rootsift(q) for q in queries], cent, proj), db, wt, sel)
        idx, val = index.rank_rows(queries, 5)
        ridx, rval = tw.rank(want, 5)
        assert np.array_equal(idx, ridx) and np.array_equal(_bits(val), _bits(rval))
        assert idx[0, 0] == 4 and idx[1, 0] == 7
        idx, val = index.rank_rows(queries[:1], 20)                        # k beyond N: the tail is unfilled
        assert np.array_equal(idx[0, :12], tw.rank(want[:1], 12)[0][0]) and (idx[0, 12:] == -1).all() and np.isneginf(val[0, 12:]).all()
        p = str(tmp_path / "asmk.npz")
        index.save(p)
        back = ASMKIndex.load(p, ctx=gpu_ctx)
        try:
            i2, v2 = back.rank_rows(queries, 5)
            assert np.array_equal(i2, ridx) and np.array_equal(_bits(v2), _bits(rval)) and back.paths == index.paths
        finally:
            back.close()
        with pytest.raises(NotImplementedError, match="rebuild"):
            index.add(["x"], [queries[0]])
    finally:
        index.close()


def test_fit_and_retrieve_return_paths(gpu_ctx):
    """three small textures through the keypoint extractor: fit trains a vocabulary on a sample of the index's own rows, and
    retrieve puts an indexed image first with a score of one (identical entries)"""
    import dsift_numpy as dtw
    from pvsim import ASMKIndex
    from pvsim.features import KeypointSIFT
    from pvsim.verify import LocalFeatureIndex
    u8 = lambda im: np.clip(np.floor(im + 0.5), 0, 255).astype(np.uint8)     # noqa: E731
    images = {name: u8(dtw.texture(160, 200, seed, channels=1)) for name, seed in (("a", 31), ("b", 32), ("c", 33))}
    ext = KeypointSIFT(ctx=gpu_ctx)
    local = LocalFeatureIndex.from_images(list(images.values()), ext, paths=list(images), ctx=gpu_ctx)
    try:
        assert local.total_rows >= 64
        index = ASMKIndex.fit(local, 16, train_rows=min(local.total_rows, 400), max_iter=5, extractor=ext)
        try:
            hits = index.retrieve(images["b"], k=2)
            assert [type(h) for h in hits] == [tuple, tuple] and hits[0][0] == "b" and hits[1][0] in ("a", "c")
            assert abs(hits[0][1] - 1.0) <= 5.5 * 2.0 ** -24 and hits[1][1] <= hits[0][1]
            assert index.n_words == 16 and index.list_sizes().sum() == len(index.ent_img)
        finally:
            index.close()
    finally:
        local.close()
