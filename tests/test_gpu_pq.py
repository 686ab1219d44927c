"""GPU tests of the compact index (csrc/pq.hip, pvsim/compact.py): every kernel against the NumPy twin (tests/pq_numpy.py),
bit for bit -- the definitions of include/pvsim.h fix each summation order, so there is no tolerance to argue about."""
import ctypes as C

import numpy as np
import pytest

import pq_numpy as tw

pytestmark = pytest.mark.gpu

SEG_ENTRIES = 40960        # table entries one LDS segment holds (160 KiB)


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _codebooks(rng, m, ksub, dsub):
    """values spanning 2^-20 .. 2^20, with codeword 1 duplicated at the end (an exact tie wherever ksub >= 3)"""
    cb = (rng.standard_normal((m, ksub, dsub)) * np.exp2(rng.integers(-20, 21, (m, ksub, 1)))).astype(np.float32)
    if ksub >= 3:
        cb[:, ksub - 1] = cb[:, 1]
    return cb


def _rows(rng, cb, n):
    """half the rows planted exactly on codewords (the duplicated one included), the others near one"""
    m, ksub, dsub = cb.shape
    pick = rng.integers(0, ksub, (n, m))
    pick[::3] = np.where(rng.random((len(pick[::3]), m)) < 0.5, ksub - 1, pick[::3])     # aim at the duplicate: the lowest j must win
    x = np.concatenate([cb[s][pick[:, s]] for s in range(m)], axis=1)
    noisy = rng.random(n) < 0.5
    x[noisy] *= (1 + 0.3 * rng.standard_normal((int(noisy.sum()), m * dsub))).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


QUANTISERS = [(1, 1, 2), (8, 8, 256), (64, 2, 256), (3, 5, 255), (16, 32, 16)]


# ------------------------------------------------------------------------------------------------ encode, table
@pytest.mark.parametrize("m,dsub,ksub", QUANTISERS)
def test_encode_matches_twin(gpu_ctx, m, dsub, ksub):
    rng = np.random.default_rng(100 + m)
    cb = _codebooks(rng, m, ksub, dsub)
    table = gpu_ctx.pq(cb)
    for n in (1, 63, 64, 65, 1000):
        x = _rows(rng, cb, n)
        d_x, d_c = _up(gpu_ctx, x), gpu_ctx.buffer(n * m + 16).fill_bytes(0x5A)
        gpu_ctx.pq_encode_dev(table, d_x.ptr, n, d_c.ptr)
        got = d_c.download((n * m + 16,), np.uint8)
        want = tw.encode(x, cb)
        assert np.array_equal(got[:n * m].reshape(n, m), want), (m, dsub, ksub, n)
        assert (got[n * m:] == 0x5A).all()
        if ksub >= 3:
            assert not (want == ksub - 1).any()          # the duplicate never wins: ties go to the lowest j
        d_x.free(), d_c.free()
    gpu_ctx.pq_encode_dev(table, None, 0, None)          # n == 0 is a no-op
    table.close()


@pytest.mark.parametrize("m,dsub,ksub", QUANTISERS)
def test_table_matches_twin(gpu_ctx, m, dsub, ksub):
    rng = np.random.default_rng(200 + m)
    cb = _codebooks(rng, m, ksub, dsub)
    table = gpu_ctx.pq(cb)
    for nq in (1, 3, 70):
        q = (rng.standard_normal((nq, m * dsub)) * np.exp2(rng.integers(-8, 9, (nq, 1)))).astype(np.float32)
        d_q, d_l = _up(gpu_ctx, q), gpu_ctx.buffer(nq * m * ksub * 4 + 16).fill_bytes(0x5A)
        gpu_ctx.pq_lut_dev(table, d_q.ptr, nq, d_l.ptr)
        got = d_l.download((nq * m * ksub + 4,), np.float32)
        assert np.array_equal(got[:-4].reshape(nq, m, ksub).view(np.uint32), tw.lut(q, cb).view(np.uint32)), (m, dsub, ksub, nq)
        assert (got[-4:].view(np.uint8) == 0x5A).all()
        d_q.free(), d_l.free()
    gpu_ctx.pq_lut_dev(table, None, 0, None)
    table.close()


# ------------------------------------------------------------------------------------------------ scan + top-k
def _scan(ctx, lut, codes, k, inv_q=None, inv_db=None, col_offset=0, merge=False, lists=None, code_offset=0):
    """code_offset: the codes start that many bytes into their (16-byte aligned, padded) buffer"""
    nq, m, ksub = lut.shape
    N = codes.shape[0]
    d_l, d_c = _up(ctx, lut), _up(ctx, codes)                      # the buffer ends at the last code
    if code_offset:
        d_c.free()
        d_c = ctx.buffer(codes.nbytes + 64).fill_bytes(0).upload(codes, offset=code_offset)
    assert d_c.ptr % 16 == 0
    d_iq = _up(ctx, inv_q) if inv_q is not None else None
    d_id = _up(ctx, inv_db) if inv_db is not None else None
    own = lists is None
    if own:
        lists = (ctx.buffer(nq * k * 8 + 64).fill_bytes(0x5A), ctx.buffer(nq * k * 4 + 64).fill_bytes(0x5A))
    d_idx, d_val = lists
    ctx.pq_scan_topk_dev(d_l.ptr, nq, m, ksub, d_c.ptr + code_offset, N, d_iq.ptr if d_iq else None, d_id.ptr if d_id else None, k, col_offset,
                         merge, d_idx.ptr, d_val.ptr)
    idx = d_idx.download((nq * k + 8,), np.int64)
    val = d_val.download((nq * k + 16,), np.float32)
    assert (idx[nq * k:].view(np.uint8) == 0x5A).all() and (val[nq * k:].view(np.uint8) == 0x5A).all()   # nothing beyond nq * k
    for b in (d_l, d_c, d_iq, d_id):
        if b is not None:
            b.free()
    return idx[:nq * k].reshape(nq, k), val[:nq * k].reshape(nq, k), lists


def _scan_case(rng, nq, m, ksub, N, coarse=False):
    """tables and codes; a third of the rows are copies of earlier rows (equal scores), `coarse` makes most scores collide"""
    lut = rng.standard_normal((nq, m, ksub)).astype(np.float32)
    if coarse:
        lut = np.round(lut).astype(np.float32)
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    if N > 2:
        dup = rng.choice(N, N // 3, replace=False)
        codes[dup] = codes[rng.integers(0, N, len(dup))]
    return lut, codes


def _check_lists(got_idx, got_val, lut, codes, k, inv_q=None, inv_db=None, col_offset=0):
    want_idx, want_val = tw.topk(tw.scores(lut, codes, inv_q, inv_db), k, col_offset)
    assert np.array_equal(got_idx, want_idx)
    assert np.array_equal(got_val.view(np.uint32), want_val.view(np.uint32))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4099])
def test_scan_topk_matches_twin(gpu_ctx, N):
    rng = np.random.default_rng(300 + N)
    for nq in (1, 3, 70):
        for m, ksub in ((8, 256), (64, 256), (3, 255), (5, 16)):      # codes in registers (m % 4 == 0, m <= 64) and the generic walk
            lut, codes = _scan_case(rng, nq, m, ksub, N)
            inv_q = (0.5 + rng.random(nq)).astype(np.float32)
            inv_db = (0.5 + rng.random(N)).astype(np.float32)
            inv_db[codes_dupes(codes)] = np.float32(1.0)                # equal factors too, so duplicated rows score equal
            for k in sorted({1, min(N, 10), min(N, 300)}):
                idx, val, lists = _scan(gpu_ctx, lut, codes, k, inv_q, inv_db)
                _check_lists(idx, val, lut, codes, k, inv_q, inv_db)
                for b in lists:
                    b.free()


def codes_dupes(codes):
    """rows whose code row occurs more than once"""
    _, inv, cnt = np.unique(codes, axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] > 1


@pytest.mark.parametrize("m,ksub", [(160, 256), (369, 111), (161, 256), (370, 111), (200, 256)])
def test_scan_at_and_across_the_lds_segment_limit(gpu_ctx, m, ksub):
    """m * ksub at the limit (160 x 256), one below (369 x 111), above (161 x 256, 370 x 111) and the two-segment walk at
    m = 200: the running sums live across the segments, so the order of the additions does not change"""
    assert (m * ksub <= SEG_ENTRIES) == ((m, ksub) in ((160, 256), (369, 111)))
    rng = np.random.default_rng(400 + m)
    N = 257
    lut, codes = _scan_case(rng, 3, m, ksub, N)
    inv_db = np.ones(N, np.float32)
    for k in (1, 10, 257):
        idx, val, lists = _scan(gpu_ctx, lut, codes, k, None, inv_db)
        _check_lists(idx, val, lut, codes, k, None, inv_db)
        for b in lists:
            b.free()


@pytest.mark.parametrize("m,ksub", [(80, 256), (176, 256), (68, 256), (67, 256), (372, 100)])
def test_scan_on_each_code_load_width(gpu_ctx, m, ksub):
    """the generic walk (m > 64) on the shapes where the shared plan gives each load width: (80, 256) width 16, one segment;
    (176, 256) width 16, two segments of 160 + 16 sub-spaces; (68, 256) width 4; (67, 256) single bytes; (372, 100) one segment
    whose size, 409 sub-spaces, is no multiple of 4: width 4 since the two scans share one rule.  The flat scan reads 4 bytes at
    a time from width 4 up; which loads a launch took cannot be seen from here, the lists are the twin's on all of them"""
    rng = np.random.default_rng(450 + m)
    N = 257
    lut, codes = _scan_case(rng, 3, m, ksub, N)
    inv_db = np.ones(N, np.float32)
    for k in (1, 10, 257):
        idx, val, lists = _scan(gpu_ctx, lut, codes, k, None, inv_db)
        _check_lists(idx, val, lut, codes, k, None, inv_db)
        for b in lists:
            b.free()


@pytest.mark.parametrize("m", [80, 64])
@pytest.mark.parametrize("code_offset", [0, 4, 1])
def test_scan_with_a_code_base_that_is_not_aligned(gpu_ctx, m, code_offset):
    """the codes start 0, 4 or 1 bytes into a 16-byte aligned buffer (padded when offset): the lists are the twin's at every
    offset, whichever load width the launcher picks from the pointer.  Which width that is cannot be seen from here (a misaligned
    load returns the same bytes); csrc/bench/scan_plan_check.cpp pins the plan: width 16 / 4 / 1 at m = 80, and at m = 64 the
    register path at offsets 0 and 4, single bytes at offset 1"""
    rng = np.random.default_rng(470 + m)
    N = 257
    lut, codes = _scan_case(rng, 3, m, 256, N)
    inv_db = (0.5 + rng.random(N)).astype(np.float32)
    inv_db[codes_dupes(codes)] = np.float32(1.0)
    for k in (1, 10, 257):
        idx, val, lists = _scan(gpu_ctx, lut, codes, k, None, inv_db, code_offset=code_offset)
        _check_lists(idx, val, lut, codes, k, None, inv_db)
        for b in lists:
            b.free()


def test_scan_equal_scores_across_panel_and_query_tile(gpu_ctx):
    """1100 queries against 4099 rows: more than one query tile (1024) and, at that many queries, panels of 4096 columns, so
    rows 4096.. merge into lists built from the first panel.  Rounded tables make most scores collide: indices ascend."""
    rng = np.random.default_rng(500)
    for m in (4, 5):                                                  # four rows per lane with the codes in registers / re-read
        lut, codes = _scan_case(rng, 1100, m, 4, 4099, coarse=True)
        codes[4096:] = codes[:3]                                      # equal scores on both sides of the panel boundary
        sc = tw.scores(lut, codes)
        assert len(np.unique(sc[0])) < 100                           # k > the number of distinct scores
        for k in (10, 300):
            idx, val, lists = _scan(gpu_ctx, lut, codes, k)          # NULL inv_q and inv_db
            _check_lists(idx, val, lut, codes, k)
            for b in lists:
                b.free()


def test_scan_two_calls_with_offset_and_merge_equal_one(gpu_ctx):
    rng = np.random.default_rng(600)
    N, cut, k, nq = 4099, 1500, 300, 3
    lut, codes = _scan_case(rng, nq, 8, 256, N, coarse=True)
    inv_q = (0.5 + rng.random(nq)).astype(np.float32)
    one_idx, one_val, lists = _scan(gpu_ctx, lut, codes, k, inv_q, None, col_offset=7)
    for b in lists:
        b.free()
    _, _, lists = _scan(gpu_ctx, lut, codes[:cut], k, inv_q, None, col_offset=7)
    two_idx, two_val, lists = _scan(gpu_ctx, lut, codes[cut:], k, inv_q, None, col_offset=7 + cut, merge=True, lists=lists)
    assert np.array_equal(two_idx, one_idx) and np.array_equal(two_val.view(np.uint32), one_val.view(np.uint32))
    _check_lists(one_idx, one_val, lut, codes, k, inv_q, None, col_offset=7)
    for b in lists:
        b.free()


def test_scan_deep_ranking_pages_through_complete_rows(gpu_ctx):
    """k > 1024: one panel of all N columns, the list is built page by page (as pvs_cosine_topk_dev); merging is refused"""
    from pvsim import _ffi
    rng = np.random.default_rng(650)
    N, k = 1203, 1100
    for nq, m, ksub in ((3, 8, 256), (2, 5, 16)):
        lut, codes = _scan_case(rng, nq, m, ksub, N, coarse=True)
        inv_db = (0.5 + rng.random(N)).astype(np.float32)
        inv_db[codes_dupes(codes)] = np.float32(1.0)
        idx, val, lists = _scan(gpu_ctx, lut, codes, k, None, inv_db, col_offset=5)
        _check_lists(idx, val, lut, codes, k, None, inv_db, col_offset=5)
        idx, val, lists2 = _scan(gpu_ctx, lut, codes, N, None, inv_db)       # the complete ranking
        _check_lists(idx, val, lut, codes, N, None, inv_db)
        for b in lists + lists2:
            b.free()
    buf = gpu_ctx.buffer(1 << 20).fill_bytes(0)
    p = buf.ptr
    st = _ffi.lib().pvs_pq_scan_topk_dev(gpu_ctx.handle, C.c_void_p(p), 1, 4, 16, C.c_void_p(p + 4096), 1200, None, None, 1100, 0, 1,
                                         C.c_void_p(p + 65536), C.c_void_p(p + 131072))
    assert st == _ffi.PVS_ERR_UNSUPPORTED
    buf.free()


# ------------------------------------------------------------------------------------------------ rescore
@pytest.mark.parametrize("d", [2, 64, 257])
def test_rescore_matches_twin(gpu_ctx, d):
    rng = np.random.default_rng(700 + d)
    N, nq = 500, 5
    X = rng.standard_normal((N, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    inv_q, inv_db = (0.5 + rng.random(nq)).astype(np.float32), (0.5 + rng.random(N)).astype(np.float32)
    d_q, d_x, d_iq, d_id = (_up(gpu_ctx, a) for a in (Q, X, inv_q, inv_db))
    for R in (1, 10, 100):
        cand = rng.integers(0, N, (nq, R)).astype(np.int64)
        if R > 1:
            cand[:, R // 2] = -1                                      # an unfilled slot
        else:
            cand[0, 0] = -1                                           # R = 1: one query's only slot unfilled, the others real
        if R > 2:
            cand[:, -1] = cand[:, 0]                                  # a repeated index
        d_c, d_v = _up(gpu_ctx, cand), gpu_ctx.buffer(nq * R * 4 + 16).fill_bytes(0x5A)
        gpu_ctx.rescore_rows_dev(d_q.ptr, nq, d_x.ptr, N, d, d_iq.ptr, d_id.ptr, d_c.ptr, R, d_v.ptr)
        got = d_v.download((nq * R + 4,), np.float32)
        want = tw.rescore(Q, X, cand, inv_q, inv_db)
        assert np.array_equal(got[:-4].reshape(nq, R).view(np.uint32), want.view(np.uint32)), (d, R)
        assert (got[-4:].view(np.uint8) == 0x5A).all()
        gpu_ctx.rescore_rows_dev(d_q.ptr, nq, d_x.ptr, N, d, None, None, d_c.ptr, R, d_v.ptr)      # NULL factors mean 1
        got = d_v.download((nq, R), np.float32)
        assert np.array_equal(got.view(np.uint32), tw.rescore(Q, X, cand).view(np.uint32))
        d_c.free(), d_v.free()
    for b in (d_q, d_x, d_iq, d_id):
        b.free()


# ------------------------------------------------------------------------------------------------ through the classes
@pytest.fixture(scope="module")
def fitted(gpu_ctx):
    """600 VLAD-like rows of L = 512 (sparse blocks, signed, L2-normalised), projected to 64 dimensions, m = 8"""
    from pvsim import CompactIndex
    rng = np.random.default_rng(800)
    basis = rng.standard_normal((24, 512)) * (rng.random((24, 512)) < 0.3)
    x = rng.standard_normal((600, 24)) @ basis + 0.2 * rng.standard_normal((600, 512))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    db = {f"img/{i:04d}.jpg": x[i] for i in range(600)}
    ci = CompactIndex.fit(db, m=8, n_components=64, ksub=64, keep_projected=True, random_state=5, ctx=gpu_ctx)
    q = (x[::40] + 0.05 * rng.standard_normal((15, 512))).astype(np.float32)
    yield ci, x, q
    ci.close()


def test_fit_projection_is_orthonormal_and_agrees_with_float64(fitted):
    ci, x, _ = fitted
    w = ci.projection
    assert w.shape == (64, 512) and w.dtype == np.float32
    assert np.abs(w.astype(np.float64) @ w.astype(np.float64).T - np.eye(64)).max() < 1e-5
    piv = np.argmax(np.abs(w), axis=1)
    assert (w[np.arange(64), piv] > 0).all()                          # sign-fixed as learn.fit_pca does
    y = ci.project(x)
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    scale = np.linalg.norm(x.astype(np.float64), axis=1)[:, None] * np.linalg.norm(w.astype(np.float64), axis=1)[None, :]
    assert (np.abs(y - ref) <= 2e-6 * scale).all()                    # the bound the f32 cosine GEMM is held to, scaled by the norms


def test_rank_equals_twin_on_the_devices_own_projection(fitted):
    ci, x, q = fitted
    codes, inv_db, proj = ci._download()
    assert np.array_equal(proj.view(np.uint32), ci.project(x).view(np.uint32))
    cb = ci.quantizer.codebooks
    assert np.array_equal(codes, tw.encode(proj, cb))
    yq = ci.project(q)
    d_y = ci.context.buffer(yq.nbytes).upload(yq)
    d_i = ci.context.buffer(len(yq) * 4)
    ci.context.row_inv_norms_dev(d_y.ptr, len(yq), yq.shape[1], d_i.ptr)
    inv_q = d_i.download((len(yq),), np.float32)
    d_y.free(), d_i.free()
    sc = tw.scores(tw.lut(yq, cb), codes, inv_q, inv_db)
    idx, val = ci.rank(q, 10)
    want_idx, want_val = tw.topk(sc, 10)
    assert np.array_equal(idx, want_idx) and np.array_equal(val.view(np.uint32), want_val.view(np.uint32))
    ridx, rval = ci.rank(q, 10, rerank=50)
    cand, _ = tw.topk(sc, 50)
    want_idx, want_val = tw.rerank(cand, tw.rescore(yq, proj, cand, inv_q, inv_db), 10)
    assert np.array_equal(ridx, want_idx) and np.array_equal(rval.view(np.uint32), want_val.view(np.uint32))
    assert np.array_equal(ridx[:, 0], np.arange(0, 600, 40))          # the exact re-ranking puts each query's source row first


def test_eval_save_load_and_nbytes(fitted, tmp_path):
    from pvsim import CompactIndex
    from pvsim import eval as ev
    ci, x, q = fitted

    class Identity:
        def encode(self, v):
            return v

    idx, val = ci.rank(q[:1], 5)
    hits = ev.retrieve_top_k_similar(q[0], ci, Identity(), k=5)
    assert [p for p, _ in hits] == [ci.paths[i] for i in idx[0]] and [s for _, s in hits] == val[0].tolist()
    ridx, _ = ci.rank(q[:1], 5, rerank=50)
    hits = ev.retrieve_top_k_similar(q[0], ci, Identity(), k=5, rerank=50)
    assert [p for p, _ in hits] == [ci.paths[i] for i in ridx[0]]
    labels = {p: i // 40 for i, p in enumerate(ci.paths)}
    assert ev.top_k_accuracy(list(q), list(range(15)), ci, labels, Identity(), k=50) > 0.9
    assert 0.0 <= ev.top_k_map(list(q), list(range(15)), ci, labels, Identity(), k=20) <= 1.0
    with pytest.raises(ValueError, match="pass k"):
        ev.top_k_map(list(q), list(range(15)), ci, labels, Identity(), k=None)
    with pytest.raises(ValueError, match="rerank=3 must be >= k=5"):
        ev.retrieve_top_k_similar(q[0], ci, Identity(), k=5, rerank=3)

    fn = str(tmp_path / "compact.npz")
    ci.save(fn)
    back = CompactIndex.load(fn, ctx=ci.context)
    assert back.paths == ci.paths and len(back) == 600
    for rr in (0, 50):
        a, b = ci.rank(q, 10, rerank=rr), back.rank(q, 10, rerank=rr)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    parts = ci.nbytes_breakdown
    assert parts["codes"] + parts["inv_norms"] == 600 * (8 + 4)
    assert ci.nbytes == 600 * (8 + 4) + 8 * 64 * 8 * 4 + 64 * 512 * 4 + 600 * 64 * 4 == back.nbytes
    back.close()


def test_fit_from_a_device_index_equals_fit_from_the_dict(gpu_ctx, fitted):
    """CompactIndex.fit(DeviceIndex) reads the resident rows in place: same projection, codebooks, codes, norms, kept rows and lists
    as the dict path, with the database as the training set and with a separate one"""
    from pvsim import CompactIndex
    from pvsim.index import DeviceIndex
    ci, x, q = fitted
    db = {p: x[i] for i, p in enumerate(ci.paths)}
    dev = DeviceIndex(db, gpu_ctx)
    a = CompactIndex.fit(dev, m=8, n_components=64, ksub=64, keep_projected=True, random_state=5)
    assert a.context is gpu_ctx and a.paths == ci.paths
    assert np.array_equal(a.projection, ci.projection) and np.array_equal(a.quantizer.codebooks, ci.quantizer.codebooks)
    for got, want in zip(a._download(), ci._download()):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    for rr in (0, 50):
        ga, gb = a.rank(q, 10, rerank=rr), ci.rank(q, 10, rerank=rr)
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1].view(np.uint32), gb[1].view(np.uint32))
    a.close()
    # a separate training set: the database rows are then projected chunk by chunk from the resident copy
    kw = dict(m=8, projection=ci.projection, ksub=64, keep_projected=True, random_state=5, train=x[::2])
    b, c = CompactIndex.fit(dev, **kw), CompactIndex.fit(db, ctx=gpu_ctx, **kw)
    for got, want in zip(b._download(), c._download()):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    gb, gc = b.rank(q, 10, rerank=20), c.rank(q, 10, rerank=20)
    assert np.array_equal(gb[0], gc[0]) and np.array_equal(gb[1].view(np.uint32), gc[1].view(np.uint32))
    b.close(), c.close(), dev.close()


def test_fit_frees_its_buffers_when_it_fails(gpu_ctx, fitted, monkeypatch):
    from pvsim import CompactIndex
    ci, x, _ = fitted
    db = {p: x[i] for i, p in enumerate(ci.paths)}
    taken, freed = [], []
    real = gpu_ctx.buffer

    def counting(nbytes):
        b = real(nbytes)
        taken.append(b)
        return b

    monkeypatch.setattr(gpu_ctx, "buffer", counting)

    def boom(*a, **k):
        raise RuntimeError("encode failed")

    monkeypatch.setattr(gpu_ctx, "pq_encode_dev", boom)
    with pytest.raises(RuntimeError, match="encode failed"):
        CompactIndex.fit(db, m=8, projection=ci.projection, ksub=64, keep_projected=True, random_state=5, ctx=gpu_ctx)
    import gc
    gc.collect()
    assert taken and all(b.ptr == 0 for b in taken)                   # every buffer the call took was given back


def test_quantizer_fit_encode_decode(gpu_ctx):
    from pvsim import ProductQuantizer
    rng = np.random.default_rng(900)
    x = rng.standard_normal((700, 12)).astype(np.float32)
    pq = ProductQuantizer(4, ksub=32, ctx=gpu_ctx).fit(x, random_state=1)
    assert pq.codebooks.shape == (4, 32, 3) and pq.codebooks.dtype == np.float32
    codes = pq.encode(x)
    assert np.array_equal(codes, tw.encode(x, pq.codebooks))
    dec = pq.decode(codes)
    assert np.array_equal(dec, tw.decode(codes, pq.codebooks))
    assert ((x - dec) ** 2).sum() < 0.5 * (x ** 2).sum()              # the quantiser learnt something
    pq.close()


# ------------------------------------------------------------------------------------------------ error paths
def test_invalid_arguments_return_an_error_without_a_launch(gpu_ctx):
    from pvsim import _ffi
    lib, h = _ffi.lib(), gpu_ctx.handle
    buf = gpu_ctx.buffer(1 << 16).fill_bytes(0)
    p = buf.ptr
    vp, null = C.c_void_p, C.c_void_p(None)

    def scan(lut=p, nq=2, m=4, ksub=16, codes=p + 4096, N=50, k=5, idx=p + 8192, val=p + 16384):
        return lib.pvs_pq_scan_topk_dev(h, vp(lut), nq, m, ksub, vp(codes), N, null, null, k, 0, 0, vp(idx), vp(val))

    assert scan() == _ffi.PVS_OK
    for bad in (dict(m=0), dict(ksub=257), dict(ksub=0), dict(k=51), dict(k=0), dict(idx=None), dict(val=None), dict(idx=p + 4),
                dict(val=p + 2), dict(lut=None), dict(codes=None), dict(N=-1)):
        assert scan(**bad) == _ffi.PVS_ERR_INVALID, bad
        assert lib.pvs_last_error()
    assert scan(nq=0, idx=None, val=None) == _ffi.PVS_OK               # nq == 0 is a no-op
    hp = C.c_void_p()
    cb = np.zeros((2, 4, 3), np.float32)
    assert lib.pvs_pq_create(h, _ffi.ptr(cb), 2, 257, 3, C.byref(hp)) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_pq_create(h, _ffi.ptr(cb), 0, 4, 3, C.byref(hp)) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_pq_create(h, null, 2, 4, 3, C.byref(hp)) == _ffi.PVS_ERR_INVALID
    table = gpu_ctx.pq(cb)
    assert lib.pvs_pq_encode_dev(h, table.handle, vp(p), 5, null) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_pq_encode_dev(h, table.handle, vp(p + 2), 5, vp(p)) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_pq_lut_dev(h, table.handle, vp(p), 5, null) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_pq_lut_dev(h, table.handle, vp(p), 5, vp(p + 1)) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_rescore_rows_dev(h, vp(p), 2, vp(p), 10, 0, null, null, vp(p), 3, vp(p)) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_rescore_rows_dev(h, vp(p), 2, vp(p), 10, 4, null, null, vp(p + 4), 3, vp(p)) == _ffi.PVS_ERR_INVALID
    assert lib.pvs_rescore_rows_dev(h, vp(p), 2, vp(p), 10, 4, null, null, vp(p), 3, null) == _ffi.PVS_ERR_INVALID
    table.close()
    gpu_ctx.sync()
    buf.free()
