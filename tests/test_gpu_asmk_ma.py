"""GPU tests of the multiple assignment of query rows in the ASMK* index: pvs_asmk_aggregate_ma_dev (csrc/asmk.hip) and
ASMKIndex.rank_rows(..., ma=) against the NumPy twin (tests/asmk_ma_numpy.py), bit for bit.

The aggregate tests use lattice inputs (centroid coordinates in 4 * {0 .. 3}, rows moved by -1, 0 or +1): every v and every residual
sum is an exact small number, so the twin's lists, ties included, are the only admissible ones."""
import numpy as np
import pytest

import asmk_ma_numpy as ma
import asmk_numpy as tw

pytestmark = pytest.mark.gpu

F = np.float32
DESC_F32, DESC_U8_ROOTSIFT = 0, 2
FILL = 0x5A
FILL32 = np.uint32(int.from_bytes(bytes([FILL] * 4), "little"))


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a) if a.nbytes else ctx.buffer(16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _lattice(rng, K, D, levels=4):
    seen = set()
    while len(seen) < K:
        seen.add(tuple((rng.randint(0, levels, D) * 4).tolist()))
    return np.array(sorted(seen), F)


def _near(rng, cent, words):
    words = np.asarray(words, np.int64)
    return (cent[words] + rng.randint(-1, 2, (len(words), cent.shape[1]))).astype(F)


def _aggregate_ma(ctx, rows_list, cent, m, proj, bits, labels=None, single=False):
    """pvs_kmeans_topm_dev (or the given labels) + pvs_asmk_aggregate_ma_dev on a batch -> (labels (total, m), words, sigs, counts,
    offsets), the slot arrays as they are.  single = True: pvs_asmk_aggregate_dev on column 0 instead (m must be 1)."""
    D, W = cent.shape[1], bits // 32
    off = np.zeros(len(rows_list) + 1, np.int64)
    np.cumsum([len(r) for r in rows_list], out=off[1:])
    total, n = int(off[-1]), len(rows_list)
    packed = np.concatenate(rows_list).astype(F) if total else np.zeros((0, D), F)
    slots = max(total * m, 4)
    cb = ctx.codebook(cent)
    bufs = [_up(ctx, packed), _up(ctx, off), ctx.buffer(slots * 4), ctx.buffer(slots * 4).fill_bytes(FILL),
            ctx.buffer(slots * 4 * W).fill_bytes(FILL), ctx.buffer(n * 4).fill_bytes(FILL)]
    d_x, d_off, d_lab, d_word, d_sig, d_cnt = bufs
    d_p = _up(ctx, proj) if proj is not None else None
    try:
        if labels is not None:
            d_lab.upload(np.ascontiguousarray(labels, dtype=np.int32))
        elif total:
            ctx.kmeans_topm_dev(cb, d_x.ptr, DESC_F32, total, m, d_lab.ptr)
        if single:
            ctx.asmk_aggregate_dev(cb, d_x.ptr, DESC_F32, d_off.ptr, off, n, total, d_lab.ptr, d_p.ptr if d_p else None, bits, d_word.ptr,
                                   d_sig.ptr, d_cnt.ptr)
        else:
            ctx.asmk_aggregate_ma_dev(cb, d_x.ptr, DESC_F32, d_off.ptr, off, n, total, d_lab.ptr, m, d_p.ptr if d_p else None, bits,
                                      d_word.ptr, d_sig.ptr, d_cnt.ptr)
        return (d_lab.download((total, m), np.int32), d_word.download((total * m,), np.int32), d_sig.download((total * m, W), np.uint32),
                d_cnt.download((n,), np.int32), off)
    finally:
        cb.close()
        for b in bufs + ([d_p] if d_p else []):
            b.free()


def _check(got, images, cent, m, proj):
    labels, words, sigs, counts, off = got
    for i, x in enumerate(images):
        lo, hi = int(off[i]), int(off[i + 1])
        want_lab = ma.topm(x, cent, m)[0] if len(x) else np.zeros((0, m), np.int32)
        assert np.array_equal(labels[lo:hi], want_lab), f"image {i}: labels"
        w, s = ma.image_entries_ma(x, want_lab, cent, proj)
        assert counts[i] == len(w), f"image {i}: {counts[i]} entries, the twin has {len(w)}"
        a, b = m * lo, m * hi                                              # the slots of image i
        assert np.array_equal(words[a:a + len(w)], w), f"image {i}: words"
        assert np.array_equal(sigs[a:a + len(w)], s), f"image {i}: signatures"
        assert (words[a + len(w):b].view(np.uint32) == FILL32).all() and (sigs[a + len(w):b] == FILL32).all(), f"image {i}: slots past the count"


def _images(rng, cent):
    K = len(cent)
    return [np.zeros((0, cent.shape[1]), F),                              # no rows
            _near(rng, cent, [K - 1]),                                    # one row
            _near(rng, cent, [3] * 70),                                   # word 3 is in the list of every row
            _near(rng, cent, rng.permutation(K)),
            _near(rng, cent, rng.randint(0, K, 300)),
            np.zeros((0, cent.shape[1]), F),
            _near(rng, cent, rng.randint(0, K, 65))]


@pytest.mark.parametrize("m", [2, 5, 8])
@pytest.mark.parametrize("D,B,with_p", [(32, 32, False), (128, 128, False), (128, 64, True)])
def test_aggregate_ma_matches_twin(gpu_ctx, D, B, with_p, m):
    rng = np.random.RandomState(2800 + D + B + m)
    cent = _lattice(rng, 40, D)
    proj = rng.standard_normal((B, D)).astype(F) if with_p else None
    images = _images(rng, cent)
    got = _aggregate_ma(gpu_ctx, images, cent, m, proj, B)
    _check(got, images, cent, m, proj)
    assert got[3][0] == 0 and got[3][1] == m and got[3][5] == 0
    shared = got[1][m * int(got[4][2]):m * int(got[4][2]) + got[3][2]]     # image 2: every row holds word 3
    assert 3 in shared.tolist()


def test_aggregate_ma_16384_keys_and_the_refusal(gpu_ctx):
    """2048 rows x 8 labels = 16384 keys are accepted, with a 128 x 128 projection, which then no longer fits beside keys and heads
    and is read from global memory; 2049 x 8 are refused, and so are 8193 rows at m = 1"""
    rng = np.random.RandomState(2900)
    cent = _lattice(rng, 48, 128, levels=2)
    proj = rng.standard_normal((128, 128)).astype(F)
    images = [_near(rng, cent, rng.randint(0, 48, 2048)), _near(rng, cent, rng.randint(0, 48, 5))]
    _check(_aggregate_ma(gpu_ctx, images, cent, 8, proj, 128), images, cent, 8, proj)
    images[1] = _near(rng, cent, rng.randint(0, 48, 2049))
    with pytest.raises(NotImplementedError, match="2049"):
        _aggregate_ma(gpu_ctx, images, cent, 8, proj, 128)
    images[1] = _near(rng, cent, rng.randint(0, 48, 8193))
    with pytest.raises(NotImplementedError, match="8193"):
        _aggregate_ma(gpu_ctx, images, cent, 1, proj, 128)
    for bad in (0, 9, 49, -1):
        with pytest.raises(ValueError, match="m must lie in"):
            _aggregate_ma(gpu_ctx, images[:1], cent, bad, proj, 128, labels=np.zeros(4, np.int32))     # refused before the labels are read


@pytest.mark.parametrize("D,B,with_p", [(32, 32, False), (128, 96, True)])
def test_aggregate_ma_at_m_1_is_the_single_assignment_kernel(gpu_ctx, D, B, with_p):
    rng = np.random.RandomState(3000 + D)
    cent = _lattice(rng, 40, D)
    proj = rng.standard_normal((B, D)).astype(F) if with_p else None
    images = _images(rng, cent) + [_near(rng, cent, rng.randint(0, 40, 8192))]
    a = _aggregate_ma(gpu_ctx, images, cent, 1, proj, B)
    b = _aggregate_ma(gpu_ctx, images, cent, 1, proj, B, labels=a[0], single=True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    _check(a, images, cent, 1, proj)


# ------------------------------------------------------------------------------------------------ end to end
def test_rank_rows_with_ma_equals_the_twin(gpu_ctx):
    """N = 200 images of uint8 rows around 30 prototypes; queries of rows whose first four ranks are clear by the twin's guard.
    rank_rows(..., ma=3) gives the twin's idx and val bits; ma=1 is the call without the argument."""
    from pvsim import ASMKIndex
    from pvsim.verify import LocalFeatureIndex
    rng = np.random.RandomState(3100)
    K, N = 30, 200
    proto = rng.randint(0, 80, (K, 128)).astype(np.uint8)
    cent = tw.rootsift(proto)

    def rows(words):
        return np.clip(proto[words].astype(np.int64) + rng.randint(-2, 3, (len(words), 128)), 0, 255).astype(np.uint8)

    images = [rows(rng.randint(0, K, rng.randint(3, 12))) for _ in range(N)]
    images[17] = np.zeros((0, 128), np.uint8)
    values = [tw.rootsift(r) for r in images]
    for x in values:
        assert tw.labels_and_gap(x, cent)[1] > 1e-3

    def query(i, clutter):
        pool = np.concatenate([images[i], rows(rng.randint(0, K, 4 * clutter))])
        return pool[ma.rank_gap_ratios(tw.rootsift(pool), cent, 3) > 1.5][:len(images[i]) + clutter]

    queries = [query(4, 3), query(111, 6), np.zeros((0, 128), np.uint8), query(199, 0)]
    qvalues = [tw.rootsift(q) for q in queries]
    for q in qvalues:
        assert ma.rank_gaps(q, cent, 3)[0] and (len(q) == 0 or tw.labels_and_gap(q, cent)[1] > 1e-3)
    assert min(len(q) for q in (queries[0], queries[1], queries[3])) >= 3

    db = tw.entries(values, cent, None)
    wt, sel = tw.word_weights(db, K), tw.selectivity(128, 3.0, 0.0)
    want3 = tw.scores(ma.entries_ma(qvalues, cent, 3, None), db, wt, sel)
    want1 = tw.scores(tw.entries(qvalues, cent, None), db, wt, sel)
    assert not np.array_equal(want3, want1)                                # the argument changes the scores

    local = LocalFeatureIndex.from_arrays(images, [np.zeros((len(r), 6), F) for r in images], [f"im{i}" for i in range(N)], ctx=gpu_ctx)
    try:
        index = ASMKIndex.build(local, cent, bits=128)
        try:
            idx, val = index.rank_rows(queries, 10, ma=3)
            ridx, rval = tw.rank(want3, 10)
            assert np.array_equal(idx, ridx) and np.array_equal(_bits(val), _bits(rval))
            i0, v0 = index.rank_rows(queries, 10)
            i1, v1 = index.rank_rows(queries, 10, ma=1)
            ridx, rval = tw.rank(want1, 10)
            assert np.array_equal(i0, ridx) and np.array_equal(_bits(v0), _bits(rval))
            assert np.array_equal(i1, i0) and np.array_equal(_bits(v1), _bits(v0))
            with pytest.raises(ValueError, match="ma must be"):
                index.rank_rows(queries, 10, ma=9)
        finally:
            index.close()
    finally:
        local.close()
