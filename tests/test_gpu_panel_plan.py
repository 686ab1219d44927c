"""The query seam of complete-row score panels (csrc/panel_plan.hpp, panel_full_rows): nq x N scores above the 1 GiB budget, so the
queries go through two blocks -- 8192 of them, then one.  Four entry points reach it, each in a single call at the smallest shape
that does: pvs_cosine_topk_f64_dev, pvs_l2_knn_dev and pvs_l2_radius_count_dev on float64 rows (N = 16384: 2^27 / N = 8192 queries
per block) and pvs_cosine_topk_dev at k = 1025 (N = 32768: 2^28 / N = 8192).

Rows hold small integers and no norms are applied, so every dot product, norm and distance is an exact integer in float32 and
float64: the same bits in any order of summation and under any split-K plan.  Exact ties are planted on both sides of the seam (the
last query of the first block and the only query of the second are one row; database rows repeat, so equal scores fall by index).
The expectation is the SAME entry point on queries that are one block by construction: the last query alone, and queries 0 and 8191
together.  Lists and values must be equal bit for bit; the radius counts must equal a NumPy count over the integer rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, K = 8193, 3
PICK = [0, NQ - 2, NQ - 1]                  # first query, last query of the first block, the query of the second block
N64, L64 = 16384, 4
N32, L32, K_DEEP = 32768, 8, 1025


@pytest.fixture(scope="module")
def ctx():
    """a context of its own: the 1 GiB panel goes back to the device when the module is done"""
    import pvsim
    c = pvsim.Context(0)
    yield c
    c.close()


def _rows(seed, nq, N, L, dtype):
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, (N, L)).astype(dtype)
    Q = rng.integers(-8, 9, (nq, L)).astype(dtype)
    X[5000] = X[N - 1] = X[17]              # equal scores against every query: decided by index
    Q[nq - 1] = Q[nq - 2]                   # one row on either side of the seam
    Q[0] = X[17]                            # a query on a database row: distance 0 three times
    return Q, X


@pytest.fixture(scope="module")
def rows64(ctx):
    Q, X = _rows(23, NQ, N64, L64, np.float64)
    dq, dx = ctx.buffer(Q.nbytes).upload(Q), ctx.buffer(X.nbytes).upload(X)
    yield Q, X, dq, dx
    dq.free()
    dx.free()


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _lists(ctx, call, d_q, nq, k, vdt):
    """call(d_q_ptr, nq, idx_ptr, val_ptr) into poisoned lists -> (idx, val)"""
    ib, vb = ctx.buffer(nq * k * 8).fill_bytes(0xFF), ctx.buffer(nq * k * np.dtype(vdt).itemsize).fill_bytes(0xFF)
    try:
        call(d_q, nq, ib.ptr, vb.ptr)
        return ib.download((nq, k), np.int64), vb.download((nq, k), vdt)
    finally:
        ib.free()
        vb.free()


def _check_seam(ctx, call, Q, d_q, N, k, vdt):
    """all NQ queries in one call against the last query alone and against queries 0 and 8191 together"""
    idx, val = _lists(ctx, call, d_q.ptr, NQ, k, vdt)
    row_bytes = Q.shape[1] * Q.itemsize
    li, lv = _lists(ctx, call, d_q.ptr + (NQ - 1) * row_bytes, 1, k, vdt)
    pair = ctx.buffer(2 * row_bytes).upload(Q[PICK[:2]])
    try:
        pi, pv = _lists(ctx, call, pair.ptr, 2, k, vdt)
    finally:
        pair.free()
    want_i, want_v = np.concatenate([pi, li]), np.concatenate([pv, lv])
    assert (want_i >= 0).all() and np.isfinite(want_v).all()
    assert np.array_equal(idx[PICK], want_i) and np.array_equal(_bits(val[PICK]), _bits(want_v))
    assert np.array_equal(idx[NQ - 1], idx[NQ - 2]) and np.array_equal(_bits(val[NQ - 1]), _bits(val[NQ - 2]))   # the tie across the seam
    assert (idx >= 0).all() and (idx < N).all() and not np.isnan(val).any()                                       # every row was written
    return idx, val


def test_f64_ranking_crosses_the_query_seam(ctx, rows64):
    Q, X, dq, dx = rows64
    idx, val = _check_seam(ctx, lambda q, nq, i, v: ctx.cosine_topk_f64_dev(q, nq, dx.ptr, N64, L64, None, None, K, i, v), Q, dq, N64,
                           K, np.float64)
    # the planted rows: query 0 is database row 17, which stands three times in the database
    s = X @ Q[0]
    order = np.lexsort((np.arange(N64), -s))[:K]
    assert np.array_equal(idx[0], order) and np.array_equal(val[0], s[order])


def test_f64_knn_crosses_the_query_seam(ctx, rows64):
    Q, X, dq, dx = rows64
    idx, dist = _check_seam(ctx, lambda q, nq, i, v: ctx.l2_knn_dev(q, nq, dx.ptr, N64, L64, True, K, i, v), Q, dq, N64, K, np.float64)
    # the planted rows: query 0 is database row 17, which stands three times in the database
    d = ((X - Q[0]) ** 2).sum(axis=1)
    order = np.lexsort((np.arange(N64), d))[:K]
    assert d[order].tolist() == [0.0, 0.0, 0.0] and {17, 5000, N64 - 1} <= set(np.flatnonzero(d == 0).tolist())
    assert np.array_equal(idx[0], order) and np.array_equal(dist[0], d[order])


def test_f64_radius_count_crosses_the_query_seam(ctx, rows64):
    Q, X, dq, dx = rows64
    r_sq = 30.0                                                              # an integer: pairs exactly on the radius count
    cb = ctx.buffer(NQ * 8).fill_bytes(0xFF)
    try:
        ctx.l2_radius_count_dev(dq.ptr, NQ, dx.ptr, N64, L64, True, r_sq, cb.ptr)
        counts = cb.download((NQ,), np.int64)
    finally:
        cb.free()
    d = ((Q[PICK][:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    want = (d <= r_sq).sum(axis=1)
    assert (d == r_sq).any() and want.min() >= 3
    assert counts[PICK].tolist() == want.tolist() and counts[NQ - 1] == counts[NQ - 2]
    assert (counts >= 0).all() and (counts <= N64).all()


def test_deep_f32_ranking_crosses_the_query_seam(ctx):
    Q, X = _rows(29, NQ, N32, L32, np.float32)
    dq, dx = ctx.buffer(Q.nbytes).upload(Q), ctx.buffer(X.nbytes).upload(X)
    try:
        _check_seam(ctx, lambda q, nq, i, v: ctx.cosine_topk_dev(q, nq, dx.ptr, N32, L32, None, None, K_DEEP, 0, 0, i, v), Q, dq,
                    N32, K_DEEP, np.float32)
    finally:
        dq.free()
        dx.free()
