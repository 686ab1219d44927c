"""GPU tests of the int8 resident index (csrc/sq8.hip, pvsim/quantized.py) against the NumPy twin (tests/sq8_numpy.py).  The dot
product of two code rows is an integer and every other step is a single float32 operation, so every comparison is on bytes."""
import numpy as np
import pytest

import sq8_numpy as tw

pytestmark = pytest.mark.gpu

OPT_SQ8_PATH = 7
PATHS = (0, 1, 2)                  # chosen by nq, the row scan, the int8 GEMM


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ encode
def _encode_rows(rng, n, L):
    """rows spanning 2^-20 .. 2^20; row 0 holds exact halves behind its amax; from five rows on: a zero row, a row with a
    subnormal amax, a one-hot row, a row of +-amax"""
    x = (rng.standard_normal((n, L)) * np.exp2(rng.integers(-20, 21, (n, 1)))).astype(np.float32)
    hx, _ = tw.exact_halves(3.0)
    x[0] = np.resize(np.concatenate([[np.float32(3.0)], hx]), L)
    if n >= 5:
        x[1] = 0
        x[2] = np.float32(1e-45) * rng.integers(-3, 4, L).astype(np.float32)
        x[2, L // 2] = np.float32(1e-45) * np.float32(-3)
        x[3] = 0
        x[3, L - 1] = np.float32(-2.5)
        x[4] = np.where(rng.random(L) < 0.5, -1, 1).astype(np.float32) * np.float32(2.0 ** 20)
    return x


@pytest.mark.parametrize("L", [1, 15, 63, 64, 65, 1000, 4100])
def test_encode_matches_twin(gpu_ctx, L):
    rng = np.random.default_rng(1000 + L)
    ld = tw.ld_of(L)
    for n in (1, 63, 64, 65, 300):
        x = _encode_rows(rng, n, L)
        d_x = _up(gpu_ctx, x)
        d_c, d_i = gpu_ctx.buffer((n + 2) * ld).fill_bytes(0x5A), gpu_ctx.buffer((n + 2) * 4).fill_bytes(0x5A)
        gpu_ctx.sq8_encode_dev(d_x.ptr, n, L, d_c.ptr, d_i.ptr)
        codes, inv = d_c.download((n + 2, ld), np.int8), d_i.download((n + 2,), np.float32)
        want_c, want_i = tw.encode(x)
        assert np.array_equal(codes[:n], want_c), (L, n, np.argwhere(codes[:n] != want_c)[:4])
        assert not codes[:n, L:].any()                                      # the padding is written, as zeros
        assert _same_bits(inv[:n], want_i), (L, n)
        assert (codes[n:].view(np.uint8) == 0x5A).all() and (inv[n:].view(np.uint8) == 0x5A).all()      # nothing past row n
        if n >= 5:
            assert not codes[1].any() and inv[1] == 0 and np.abs(codes[2]).max() == 127 and np.abs(codes[4, :L]).min() == 127
        for b in (d_x, d_c, d_i):
            b.free()
    gpu_ctx.sq8_encode_dev(None, 0, L, None, None)                          # n == 0 is a no-op


def test_encode_half_row_rounds_to_even(gpu_ctx):
    hx, ht = tw.exact_halves(3.0)
    k = np.floor(ht).astype(np.int64)
    assert (k % 2 == 0).any() and (k % 2 == 1).any() and (ht > 0).any() and (ht < 0).any()
    x = np.concatenate([[np.float32(3.0)], hx])[None, :]
    d_x, d_c, d_i = _up(gpu_ctx, x), gpu_ctx.buffer(tw.ld_of(x.shape[1])), gpu_ctx.buffer(16)
    gpu_ctx.sq8_encode_dev(d_x.ptr, 1, x.shape[1], d_c.ptr, d_i.ptr)
    got = d_c.download((tw.ld_of(x.shape[1]),), np.int8)[1:x.shape[1]]
    assert np.array_equal(got, np.where(k % 2 == 0, k, k + 1))
    for b in (d_x, d_c, d_i):
        b.free()


# ------------------------------------------------------------------------------------------------ scores and lists
def _code_rows(nq, N, L):
    """asymmetric integer rows: Q[i][t] and X[j][t] follow different patterns, so a swapped row / column or a wrong k map shows.
    Planted: duplicated database rows (exact ties, decided by the index) and, where 127^2 L exceeds 2^24, two rows whose sums with
    query 0 differ by one and collapse to one float."""
    ld = tw.ld_of(L)
    t = np.arange(L, dtype=np.int64)[None, :]
    i, j = np.arange(nq, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[:, None]
    qc, dc = np.zeros((nq, ld), np.int8), np.zeros((N, ld), np.int8)
    qc[:, :L] = (7 * i + 3 * t + (i * t) % 5) % 255 - 127
    dc[:, :L] = (11 * j + 5 * t + (j * t) % 3) % 253 - 126
    if N >= 4:
        dc[N - 1], dc[2] = dc[0], dc[1]
    collapse = L >= 2000 and N >= 10
    if collapse:
        qc[0, :L], dc[5, :L], dc[9, :L] = 127, 127, 127
        qc[0, L - 1], dc[5, L - 1], dc[9, L - 1] = 1, 5, 4
    iq, idb = tw.factors(qc), tw.factors(dc)
    if collapse:
        idb[9] = idb[5]                            # the entry point takes the factors it is given: equal ones leave the sums to decide
        a = tw.acc(qc[:1], dc[[5, 9]])[0]
        assert a[0] == a[1] + 1 and a[1] > 2 ** 24 and np.float32(np.int32(a[0])) == np.float32(np.int32(a[1]))
    return qc, iq, dc, idb


def _topk_gpu(ctx, d_qc, d_iq, nq, d_dc, d_idb, N, L, k, col_offset=0, merge=False, out=None):
    d_idx, d_val = out or (ctx.buffer(nq * k * 8), ctx.buffer(nq * k * 4))
    ctx.sq8_topk_dev(d_qc.ptr, d_iq.ptr, nq, d_dc.ptr if hasattr(d_dc, "ptr") else d_dc, d_idb.ptr if hasattr(d_idb, "ptr") else d_idb,
                     N, L, k, col_offset, merge, d_idx.ptr, d_val.ptr)
    got = d_idx.download((nq, k), np.int64), d_val.download((nq, k), np.float32)
    if out is None:
        d_idx.free(), d_val.free()
    return got


@pytest.mark.parametrize("nq", [1, 4, 5, 31, 32, 33, 129])
@pytest.mark.parametrize("L", [1, 64, 65, 1000, 4100])
def test_lists_match_twin_on_every_path(gpu_ctx, L, nq):
    for N in (1, 127, 128, 129, 1000):
        qc, iq, dc, idb = _code_rows(nq, N, L)
        score = tw.scores(qc, iq, dc, idb)
        bufs = [_up(gpu_ctx, a) for a in (qc, iq, dc, idb)]
        for k in sorted({kk for kk in (1, 16, 17, 100, N) if kk <= N}):
            want_i, want_v = tw.topk(score, k)
            for path in PATHS:
                with gpu_ctx.option(OPT_SQ8_PATH, path):
                    got_i, got_v = _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2], bufs[3], N, L, k)
                assert np.array_equal(got_i, want_i), (L, nq, N, k, path, np.argwhere(got_i != want_i)[:4])
                assert _same_bits(got_v, want_v), (L, nq, N, k, path)
        if N >= 4:                                 # the planted ties are exact and stand in index order (checked above at k = N)
            pos = {int(c): p for p, c in enumerate(tw.topk(score, N)[0][0])}
            pairs = [(0, N - 1), (1, 2)] + ([(5, 9)] if L >= 2000 and N >= 10 else [])
            for lo, hi in pairs:
                assert score[0, lo].view(np.uint32) == score[0, hi].view(np.uint32) and pos[lo] < pos[hi]
        for b in bufs:
            b.free()


def test_largest_sum_on_both_paths(gpu_ctx):
    L = tw.MAX_L
    t = np.arange(L)
    s0 = np.where(t % 3 == 0, -127, 127).astype(np.int8)
    s1 = np.where((t // 7) % 2 == 0, -127, 127).astype(np.int8)
    qc, dc = np.stack([s0, s1]), np.stack([s0, -s0, s1])
    a = tw.acc(qc, dc)
    assert a[0, 0] == 127 * 127 * L == 2114060288 and a[0, 1] == -2114060288 and a[1, 2] == 2114060288
    iq, idb = tw.factors(qc), tw.factors(dc)
    want_i, want_v = tw.topk(tw.scores(qc, iq, dc, idb), 3)
    bufs = [_up(gpu_ctx, x) for x in (qc, iq, dc, idb)]
    ones = _up(gpu_ctx, np.ones(3, np.float32))            # factors of one: the scores are the converted sums themselves
    for path in PATHS:
        with gpu_ctx.option(OPT_SQ8_PATH, path):
            got_i, got_v = _topk_gpu(gpu_ctx, bufs[0], bufs[1], 2, bufs[2], bufs[3], 3, L, 3)
            raw_i, raw_v = _topk_gpu(gpu_ctx, bufs[0], ones, 2, bufs[2], ones, 3, L, 3)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), path
        assert raw_v[0, 0] == np.float32(2114060288) and raw_v[0, 2] == np.float32(-2114060288) and raw_i[0].tolist() == [0, 2, 1], path
    for b in bufs + [ones]:
        b.free()


def test_more_than_one_panel(gpu_ctx):
    """1024 x 4100 scores exceed one panel (2^22 floats): two column blocks, merged inside the call"""
    nq, N, L, k = 1024, 4100, 64, 10
    qc, iq, dc, idb = _code_rows(nq, N, L)
    want_i, want_v = tw.topk(tw.scores(qc, iq, dc, idb), k)
    bufs = [_up(gpu_ctx, a) for a in (qc, iq, dc, idb)]
    for path in PATHS:
        with gpu_ctx.option(OPT_SQ8_PATH, path):
            got_i, got_v = _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2], bufs[3], N, L, k)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), path
    for b in bufs:
        b.free()


def test_merge_over_two_halves_equals_one_call(gpu_ctx):
    nq, N, L, k = 33, 1000, 65, 17
    ld = tw.ld_of(L)
    qc, iq, dc, idb = _code_rows(nq, N, L)
    want = tw.topk(tw.scores(qc, iq, dc, idb), k)
    bufs = [_up(gpu_ctx, a) for a in (qc, iq, dc, idb)]
    half = 437
    for path in PATHS:
        with gpu_ctx.option(OPT_SQ8_PATH, path):
            one = _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2], bufs[3], N, L, k)
            out = (gpu_ctx.buffer(nq * k * 8), gpu_ctx.buffer(nq * k * 4))
            _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2].ptr, bufs[3].ptr, half, L, k, 0, False, out)
            two = _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2].ptr + half * ld, bufs[3].ptr + half * 4, N - half, L, k, half, True, out)
        for got in (one, two):
            assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), path
        out[0].free(), out[1].free()
    for b in bufs:
        b.free()


def test_ranking_deeper_than_1024(gpu_ctx):
    nq, N, L, k = 3, 1500, 65, 1100
    qc, iq, dc, idb = _code_rows(nq, N, L)
    want = tw.topk(tw.scores(qc, iq, dc, idb), k)
    bufs = [_up(gpu_ctx, a) for a in (qc, iq, dc, idb)]
    got = _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2], bufs[3], N, L, k)
    assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1])
    with pytest.raises(NotImplementedError):
        _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2], bufs[3], N, L, k, 0, True)
    with pytest.raises(ValueError):
        _topk_gpu(gpu_ctx, bufs[0], bufs[1], nq, bufs[2], bufs[3], N, L, N + 1)
    with pytest.raises(ValueError):
        gpu_ctx.sq8_topk_dev(bufs[0].ptr, bufs[1].ptr, nq, bufs[2].ptr, bufs[3].ptr, N, tw.MAX_L + 1, 1, 0, False, bufs[0].ptr, bufs[1].ptr)
    with pytest.raises(ValueError):
        gpu_ctx.set_option(OPT_SQ8_PATH, 3)
    for b in bufs:
        b.free()


# ------------------------------------------------------------------------------------------------ class level
def _rows(rng, n, L):
    x = (rng.standard_normal((n, L)) * np.exp2(rng.integers(-6, 7, (n, 1)))).astype(np.float32)
    return x


def _map(x, first=0):
    return {f"img/{first + i:04d}.png": x[i] for i in range(x.shape[0])}


def _assert_equals_fresh(index, survivors: dict, q, ctx):
    """codes and factors equal those of a fresh build from the survivors (and the twin's), and rank equals the twin on them"""
    import pvsim
    x = np.array(list(survivors.values()))
    codes, inv = index._download()
    want_c, want_i = tw.encode(x)
    assert index.keys() == list(survivors.keys()) and len(index) == len(survivors)
    assert np.array_equal(codes, want_c) and _same_bits(inv, want_i)
    fresh = pvsim.Int8Index(survivors, ctx)
    fc, fi = fresh._download()
    assert np.array_equal(codes, fc) and _same_bits(inv, fi)
    fresh.close()
    k = min(7, len(survivors))
    got_i, got_v = index.rank(q, k)
    want = tw.rank(q, x, k)
    assert np.array_equal(got_i, want[0]) and _same_bits(got_v, want[1])


def test_index_construction_and_rank(gpu_ctx):
    import pvsim
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(5)
    x, q = _rows(rng, 40, 70), _rows(rng, 6, 70)
    x[7] = x[3] * np.float32(4.0)                            # the scale cancels: an exact tie, decided by the index
    m = _map(x)
    a = pvsim.Int8Index(m, gpu_ctx)
    dense = DeviceIndex(m, gpu_ctx)
    b = pvsim.Int8Index.from_index(dense)
    (ac, ai), (bc, bi) = a._download(), b._download()
    assert np.array_equal(ac, bc) and _same_bits(ai, bi) and ac.shape == (40, 128)
    assert np.array_equal(dense.matrix, x) and len(dense) == 40      # the DeviceIndex is left as it is
    assert a.shape == (40, 70) and len(a) == 40 and a.paths == list(m) and a.keys() == list(m)
    assert a.nbytes_breakdown == {"codes": 40 * 128, "factors": 160} and a.nbytes == 40 * 132
    _assert_equals_fresh(a, m, q, gpu_ctx)
    for nq in (1, 6):                                        # the row scan and the matrix kernel behind the same method
        got = b.rank(q[:nq], 40)
        want = tw.rank(q[:nq], x, 40)
        assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1])
    assert a.rank(q[:0], 3)[0].shape == (0, 3)
    with pytest.raises(TypeError, match="float64"):
        a.rank(q.astype(np.float64), 3)
    with pytest.raises(ValueError):
        a.rank(q, 41)
    with pytest.raises(ValueError):
        a.rank(q[:, :69], 3)
    bad = q.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        a.rank(bad, 3)
    with pytest.raises(TypeError):
        pvsim.Int8Index.from_index(DeviceIndex({p: v.astype(np.float64) for p, v in m.items()}, gpu_ctx))
    for ix in (a, b, dense):
        ix.close()


def test_index_updates_equal_a_fresh_build(gpu_ctx):
    import pvsim
    rng = np.random.default_rng(6)
    x, q = _rows(rng, 23, 65), _rows(rng, 5, 65)
    live = _map(x[:12])
    index = pvsim.Int8Index(live, gpu_ctx)
    _assert_equals_fresh(index, live, q, gpu_ctx)

    new = _map(x[12:15], 12)                                 # add 3
    index.add(new)
    live.update(new)
    _assert_equals_fresh(index, live, q, gpu_ctx)

    first, last = list(live)[0], list(live)[-1]              # remove 2: the first and the last
    index.remove([last, first])
    del live[first], live[last]
    _assert_equals_fresh(index, live, q, gpu_ctx)

    new = _map(x[15:16], 15)                                 # add 1
    index.add(new)
    live.update(new)
    _assert_equals_fresh(index, live, q, gpu_ctx)

    index.reserve(4 * index.capacity + 5)                    # beyond the capacity: the buffers move
    assert index.capacity >= 4 * 12 and len(index) == len(live)
    _assert_equals_fresh(index, live, q, gpu_ctx)

    middle = list(live)[len(live) // 2]                      # remove a middle row
    del index[middle]
    del live[middle]
    _assert_equals_fresh(index, live, q, gpu_ctx)

    from pvsim.index import DeviceIndex                      # resident rows are read in place
    more = _map(x[16:23], 16)
    dense = DeviceIndex(more, gpu_ctx)
    index.add(dense)
    live.update(more)
    _assert_equals_fresh(index, live, q, gpu_ctx)
    dense.close()

    before = index._download()                               # the error cases change nothing
    some = list(live)[3]
    with pytest.raises(ValueError, match="already indexed"):
        index.add({"img/new.png": x[0], some: x[1]})
    with pytest.raises(KeyError):
        index.remove([some, "img/none.png"])
    with pytest.raises(ValueError, match="named twice"):
        index.remove([some, some])
    with pytest.raises(ValueError):
        index.add({"img/new.png": x[0, :64]})
    with pytest.raises(TypeError):
        index.add({"img/new.png": x[0].astype(np.float64)})
    with pytest.raises(ValueError, match="NaN"):
        index.add({"img/new.png": np.full(65, np.inf, np.float32)})
    after = index._download()
    assert np.array_equal(before[0], after[0]) and _same_bits(before[1], after[1]) and index.keys() == list(live)
    _assert_equals_fresh(index, live, q, gpu_ctx)
    index.close()


def test_index_save_and_load(gpu_ctx, tmp_path):
    import pvsim
    rng = np.random.default_rng(7)
    x, q = _rows(rng, 30, 100), _rows(rng, 4, 100)
    index = pvsim.Int8Index(_map(x), gpu_ctx)
    fn = str(tmp_path / "int8.npz")
    index.save(fn)
    with np.load(fn, allow_pickle=False) as z:
        assert z["codes"].shape == (30, 100) and z["codes"].dtype == np.int8 and str(z["kind"]) == "int8_index"
    back = pvsim.Int8Index.load(fn, gpu_ctx)
    (c0, i0), (c1, i1) = index._download(), back._download()
    assert np.array_equal(c0, c1) and _same_bits(i0, i1) and back.keys() == index.keys() and back.shape == (30, 100)
    a, b = index.rank(q, 9), back.rank(q, 9)
    assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1])
    with pytest.raises(ValueError):
        pvsim.CompactIndex.load(fn, gpu_ctx)
    index.close(), back.close()


def test_eval_ranks_through_the_index(gpu_ctx):
    import pvsim
    from pvsim import eval as ev
    from pvsim.encoders import VLADEncoder
    from pvsim.features import Lambda
    from pvsim.models import KMeansModel
    rng = np.random.default_rng(8)
    centres = rng.standard_normal((4, 8)).astype(np.float32) * 40 + 128
    enc = VLADEncoder(Lambda(lambda im: im[:, :, 0].astype(np.float32), 8), kmeans_model=KMeansModel(centres), context=gpu_ctx)
    images = [rng.integers(0, 256, (int(rng.integers(5, 30)), 8, 3)).astype(np.uint8) for _ in range(25)]      # rows of plane 0: descriptors
    vecs = np.vstack([enc.encode(im).reshape(1, -1) for im in images]).astype(np.float32)
    paths = [f"img/{i}.png" for i in range(25)]
    index = pvsim.Int8Index(dict(zip(paths, vecs)), gpu_ctx)
    query = images[11]
    qv = enc.encode(query).reshape(1, -1).astype(np.float32)
    want_i, want_v = tw.rank(qv, vecs, 5)
    hits = ev.retrieve_top_k_similar(query, index, enc, k=5)
    assert [p for p, _ in hits] == [paths[i] for i in want_i[0]] and hits[0][0] == paths[11]
    assert [np.float32(s) for _, s in hits] == want_v[0].tolist()
    labels = {p: i % 5 for i, p in enumerate(paths)}
    assert ev.top_k_accuracy(images[:6], [i % 5 for i in range(6)], index, labels, enc, k=1) == 1.0
    assert ev.top_k_map(images[:6], [i % 5 for i in range(6)], index, labels, enc, k=25) > 0
    with pytest.raises(ValueError, match="pass k"):
        ev.top_k_map(images[:2], [0, 1], index, labels, enc, k=None)
    for kw in (dict(expand=pvsim.QueryExpansion()), dict(rerank=10), dict(nprobe=2), dict(diffuse=object()), dict(reciprocal=object())):
        with pytest.raises(ValueError, match=next(iter(kw)) + "= needs"):
            ev.retrieve_top_k_similar(query, index, enc, k=5, **kw)
    index.close()
