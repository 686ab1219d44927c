"""The image-clustering device code (csrc/neighbors.hip, its use of topk.hip and of the f64 GEMM, and the device blocks of the
spectral solver in pvsim/cluster.py) against the float64 restatements of tests/neighbors_numpy.py, at the shapes where its indexing
changes path: separate query rows, a last column panel shorter than k, the query-tile seams of the float32 and float64 passes, every
branch of the candidate slots, k = 1, k = N and k beyond the prefilter (bare and paged float64 ranking), rows too large for float32
keys, an unaligned base pointer, overflowing candidate lists, the radius passes with their cursor offsets, the block product and the
transpose at ragged sizes, and the eigensolver against a dense decomposition.

Inputs are LATTICE rows (tests/neighbors_cases.py: small seeded integers as float32 or float64): every product, norm, key and
distance is an exact integer or half-integer in both formats, so the device must EQUAL the restatement -- indices and squared
distances, np.array_equal, on every path.  Exact ties are frequent, so a wrong tie order or a candidate dropped at a seam shows.
tests/test_neighbors_host.py asserts on the same rows the conditions used here (candidate counts within the slots, pairs exactly on
the radius, spectral gaps).  Only the eigensolver keeps a tolerance, derived from its stopping rule."""
import functools
import warnings

import numpy as np
import pytest

import neighbors_cases as nc
import neighbors_numpy as nn
from pvsim import cluster

pytestmark = pytest.mark.gpu


def _up(ctx, a, offset=0):
    """rows on the device, `offset` bytes into their buffer -> (buffer, device address of the rows)"""
    a = np.ascontiguousarray(a)
    b = ctx.buffer(a.nbytes + offset).upload(a, offset)
    return b, b.ptr + offset


def _knn(ctx, Q, X, k, x_offset=0):
    """pvs_l2_knn_dev on host rows; Q is X (the same object) passes one device pointer for both -> (idx, squared distances, stats)"""
    xb, xp = _up(ctx, X, x_offset)
    qb, qp = (xb, xp) if Q is X else _up(ctx, Q)
    nq = len(Q)
    ib, db = ctx.buffer(nq * k * 8).fill_bytes(0xFF), ctx.buffer(nq * k * 8).fill_bytes(0xFF)
    try:
        st = ctx.l2_knn_dev(qp, nq, xp, len(X), X.shape[1], X.dtype == np.float64, k, ib.ptr, db.ptr, stats=True)
        return ib.download((nq, k), np.int64), db.download((nq, k), np.float64), st
    finally:
        for b in {xb, qb, ib, db}:
            b.free()


def _radius(ctx, Q, X, r_sq, with_sq=True):
    """count, host prefix sum, fill -> (indptr, indices, squared distances or None)"""
    xb, xp = _up(ctx, X)
    qb, qp = (xb, xp) if Q is X else _up(ctx, Q)
    nq, f64 = len(Q), X.dtype == np.float64
    cb = ctx.buffer(nq * 8).fill_bytes(0xFF)
    bufs = {xb, qb, cb}
    try:
        ctx.l2_radius_count_dev(qp, nq, xp, len(X), X.shape[1], f64, r_sq, cb.ptr)
        indptr = np.zeros(nq + 1, np.int64)
        np.cumsum(cb.download((nq,), np.int64), out=indptr[1:])
        nnz = int(indptr[-1])
        pb = ctx.buffer((nq + 1) * 8).upload(indptr)
        ib, db = ctx.buffer((nnz + 1) * 8).fill_bytes(0xFF), ctx.buffer((nnz + 1) * 8).fill_bytes(0xFF)
        bufs |= {pb, ib, db}
        ctx.l2_radius_fill_dev(qp, nq, xp, len(X), X.shape[1], f64, r_sq, pb.ptr, ib.ptr, db.ptr if with_sq else None)
        assert ib.download((1,), np.int64, nnz * 8)[0] == -1                 # nothing written past the last entry
        return indptr, ib.download((nnz,), np.int64), db.download((nnz,), np.float64) if with_sq else None
    finally:
        for b in bufs:
            b.free()


@functools.lru_cache(maxsize=None)
def _want_knn(table, name, f64):
    Q, X, k = nc.knn_rows(name, np.float64 if f64 else np.float32, getattr(nc, table))
    return nn.knn_lists(Q, X, k)


@functools.lru_cache(maxsize=None)
def _want_seam_radius():
    return nn.radius_csr(*nc.radius_seam_rows())


def _assert_lists(got_idx, got_sq, want):
    assert np.array_equal(got_idx, want[0])
    assert np.array_equal(got_sq, want[1])


# ================================================================================ kNN: the prefilter and its slots
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(set(nc.KNN_FILTERED) - {"margin_L256"}))
def test_knn_lists_equal_the_restatement(gpu_ctx, name, dtype):
    """float32 rows: the prefilter ran, no list overflowed, and it kept exactly the restated candidates (the sum over the queries of
    the columns within the margin of the running k-th key) in the restated number of slots"""
    Q, X, k = nc.knn_rows(name, dtype)
    idx, sq, st = _knn(gpu_ctx, Q, X, k)
    _assert_lists(idx, sq, _want_knn("KNN_FILTERED", name, dtype == np.float64))
    if dtype == np.float32:
        counts, cap = nn.candidate_counts(Q, X, k, same=Q is X)
        assert st == {"filtered": True, "overflowed": 0, "candidates": int(counts.sum()), "slots": cap}, st
    else:
        assert not st["filtered"]


def test_knn_margin_follows_the_gemm_kernel_that_ran(gpu_ctx):
    """The same rows 16-byte aligned (MFMA GEMM, chains of 1024) and 4 bytes into their buffer (generic tile GEMM, one chain of
    L fma): the lists are the restatement's both times, and the candidate total is the one of the chain term that applies -- the
    two differ on these rows (asserted in tests/test_neighbors_host.py)"""
    Q, X, k = nc.knn_rows("margin_L256")
    L = X.shape[1]
    assert L % 4 == 0
    want = _want_knn("KNN_FILTERED", "margin_L256", False)
    for offset, generic in ((0, False), (4, True)):
        idx, sq, st = _knn(gpu_ctx, Q, X, k, x_offset=offset)
        _assert_lists(idx, sq, want)
        counts, cap = nn.candidate_counts(Q, X, k, chain=nn.chain_term(L, generic=generic))
        assert st == {"filtered": True, "overflowed": 0, "candidates": int(counts.sum()), "slots": cap}, (offset, st)


# ================================================================================ kNN: beyond the prefilter
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["k257", "k300", "paged"])
def test_knn_deeper_than_the_prefilter_equals_the_restatement(gpu_ctx, name, dtype):
    """k > 256: the bare float64 ranking of -d, negated back; `paged` pages through rows longer than the ranking's buffer"""
    Q, X, k = nc.knn_rows(name, dtype, nc.KNN_F64)
    idx, sq, st = _knn(gpu_ctx, Q, X, k)
    _assert_lists(idx, sq, _want_knn("KNN_F64", name, dtype == np.float64))
    assert st["filtered"] is False and st["candidates"] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_knn_across_the_float64_query_tile_seam(gpu_ctx, dtype):
    """70000 queries x 2000 rows: float64 panels of 67108 queries.  float64 rows take them directly (every query re-scored: at most
    19 rows tie at or below its k-th); float32 rows of the same values take the 8192-query tiles of the prefilter"""
    Q, X, k = nc.knn_rows("seam", dtype, nc.KNN_F64)
    idx, sq, st = _knn(gpu_ctx, Q, X, k)
    want = _want_knn("KNN_F64", "seam", True)
    tail = slice(nc.SEAM_QT - 2, None)
    assert np.array_equal(idx[tail], want[0][tail]) and np.array_equal(sq[tail], want[1][tail])     # the seam first: a short report
    _assert_lists(idx, sq, want)
    assert st["filtered"] == (dtype == np.float32) and st["overflowed"] == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_knn_of_rows_too_large_for_float32_keys(gpu_ctx, dtype):
    """rows scaled by 2^51: |row|^2 > 2^100, so float32 rows skip the prefilter; every float64 value is the unscaled integer times
    2^102, so the lists are those of the unscaled rows"""
    Q, X, k = nc.knn_rows("huge", dtype, nc.KNN_F64)
    s = dtype(nc.HUGE_SCALE)
    idx, sq, st = _knn(gpu_ctx, Q * s, X * s, k)
    want = _want_knn("KNN_F64", "huge", dtype == np.float64)
    assert np.array_equal(idx, want[0])
    assert np.array_equal(sq, want[1] * nc.HUGE_SCALE ** 2)
    assert st["filtered"] is False


@pytest.mark.parametrize("separate", [False, True], ids=["self", "queries"])
def test_knn_overflowing_lists_equal_the_restatement(gpu_ctx, separate):
    """300 identical rows + 400 distinct ones, float32: the identical rows overflow their 256 slots, the call redoes everything in
    float64, where they overflow again and keep the GEMM's ranking while the other queries are re-scored.  On lattice rows both
    rankings are exact: every list equals the restatement.  `queries`: the same rows from a second buffer (Q != X)"""
    X, k = nc.overflow_rows()
    Q = X.copy() if separate else X
    idx, sq, st = _knn(gpu_ctx, Q, X, k)
    assert st["filtered"] and st["overflowed"] >= 300 and st["slots"] == 256
    _assert_lists(idx, sq, nn.knn_lists(X, X, k))
    assert np.array_equal(idx[:300], np.tile(np.arange(k), (300, 1))) and not sq[:300].any()


def test_knn_repeats_bit_for_bit_on_grown_workspace(gpu_ctx):
    Q, X, k = nc.knn_rows("k129")
    first = _knn(gpu_ctx, Q, X, k)
    small = nc.knn_rows("tiny_9")
    _knn(gpu_ctx, *small)
    again = _knn(gpu_ctx, Q, X, k)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    Q64, X64, _ = nc.knn_rows("k129", np.float64)
    a, b = _knn(gpu_ctx, Q64, X64, k), _knn(gpu_ctx, Q64, X64, k)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(a[0], first[0]) and np.array_equal(a[1], first[1])


# ================================================================================ radius neighbours
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_neighbors_of_the_rows_themselves(gpu_ctx, dtype):
    """pvsim.cluster.radius_neighbors: eps = 5 with pairs at squared distance exactly 25 (d <= r keeps them), with and without the
    distances; eps = 0 returns each row with its exact duplicates"""
    X, eps = nc.radius_self_rows(dtype)
    want = nn.radius_csr(X, X, float(eps * eps))
    assert (want[2] == eps * eps).sum() > 0
    indptr, indices, dist = cluster.radius_neighbors(X, eps, ctx=gpu_ctx, return_distance=True)
    assert np.array_equal(indptr, want[0]) and np.array_equal(indices, want[1])
    assert np.array_equal(dist, np.sqrt(want[2]))
    indptr, indices = cluster.radius_neighbors(X, eps, ctx=gpu_ctx)
    assert np.array_equal(indptr, want[0]) and np.array_equal(indices, want[1])
    want0 = nn.radius_csr(X, X, 0.0)
    assert want0[0][-1] == len(X) + 12                          # six planted pairs
    indptr, indices, dist = cluster.radius_neighbors(X, 0, ctx=gpu_ctx, return_distance=True)
    assert np.array_equal(indptr, want0[0]) and np.array_equal(indices, want0[1]) and not dist.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_neighbors_of_separate_queries(gpu_ctx, dtype):
    Q, X, r = nc.radius_query_rows(dtype)
    want = nn.radius_csr(Q, X, r)
    assert (want[2] == r).sum() > 0
    for with_sq in (True, False):
        indptr, indices, sq = _radius(gpu_ctx, Q, X, r, with_sq)
        assert np.array_equal(indptr, want[0]) and np.array_equal(indices, want[1])
        assert sq is None or np.array_equal(sq, want[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_passes_across_the_query_tile_seam(gpu_ctx, dtype):
    """70000 queries x 2000 rows, r^2 = 30: the count and the fill both run two panels (67108 + 2892 queries); the cursors, the query
    norms and the CSR offsets of the second panel start at query 67108"""
    Q, X, r = nc.radius_seam_rows(dtype)
    want = _want_seam_radius()
    indptr, indices, sq = _radius(gpu_ctx, Q, X, r)
    assert np.array_equal(indptr, want[0])
    at = want[0][nc.SEAM_QT - 2]
    assert np.array_equal(indices[at:], want[1][at:]) and np.array_equal(sq[at:], want[2][at:])     # the seam first: a short report
    assert np.array_equal(indices, want[1]) and np.array_equal(sq, want[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_radius_rows_without_a_neighbour(gpu_ctx, dtype):
    """far-away queries between near ones: indptr repeats; only far-away queries: nnz = 0"""
    _, X, r = nc.radius_query_rows(dtype)
    far = np.full((1, X.shape[1]), 50, dtype)
    Q = np.concatenate([far, X[:2], far, far, X[5:6], far])
    want = nn.radius_csr(Q, X, r)
    assert np.array_equal(np.diff(want[0]) == 0, [True, False, False, True, True, False, True])
    indptr, indices, sq = _radius(gpu_ctx, Q, X, r)
    assert np.array_equal(indptr, want[0]) and np.array_equal(indices, want[1]) and np.array_equal(sq, want[2])
    indptr, indices, sq = _radius(gpu_ctx, np.concatenate([far, -far]), X, r)
    assert np.array_equal(indptr, [0, 0, 0]) and len(indices) == 0


# ================================================================================ the solver's blocks
def _csr(rng, n):
    """seeded CSR with empty rows, one row holding every column, unsorted columns, dyadic values"""
    rows = []
    for i in range(n):
        if i % 3 == 1 and n > 1:
            cols = np.zeros(0, np.int64)                                       # an empty row
        elif i == n // 2:
            cols = rng.permutation(n)                                          # every column, unsorted
        else:
            cols = rng.permutation(n)[:rng.integers(1, min(n, 9) + 1)]         # a few columns, unsorted
        rows.append(cols.astype(np.int64))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(c) for c in rows], out=indptr[1:])
    indices = np.concatenate(rows)
    data = rng.integers(-8, 9, len(indices)) / 4.0
    return indptr, indices, data


@pytest.mark.parametrize("m", [1, 63, 64, 65, 153])
@pytest.mark.parametrize("n", [1, 5, 259])
def test_spmm_equals_the_restatement(gpu_ctx, n, m):
    """Y = alpha S X + X diag(beta) + gamma Z on dyadic values (every product and sum exact): the four beta / Z combinations, and
    alpha = 0 with both, the residual form of the solver; m > 64 needs the second pass of the lanes, n % 4 != 0 a ragged block"""
    rng = np.random.default_rng(1000 * n + m)
    indptr, indices, data = _csr(rng, n)
    X, Z = rng.integers(-9, 10, (n, m)).astype(np.float64), rng.integers(-9, 10, (n, m)).astype(np.float64)
    beta = rng.integers(-6, 7, m) / 2.0
    bufs = [_up(gpu_ctx, a)[0] for a in (indptr, indices, data, X, Z, beta)]
    ip, ix, dx, xb, zb, bb = bufs
    yb = gpu_ctx.buffer(n * m * 8)
    bufs.append(yb)
    try:
        for alpha, b, z, gamma in ((1.5, None, None, 0.0), (-0.75, beta, None, 0.0), (2.0, None, Z, -1.0), (0.5, beta, Z, 0.25),
                                   (0.0, beta, Z, 1.0), (1.0, None, None, 3.0)):
            yb.fill_bytes(0xFF)
            gpu_ctx.csr_spmm_f64_dev(n, ip.ptr, ix.ptr, dx.ptr, xb.ptr, m, yb.ptr, alpha, bb.ptr if b is not None else None,
                                     zb.ptr if z is not None else None, gamma)
            want = nn.spmm(indptr, indices, data, X, alpha, b, z, gamma)
            assert np.array_equal(yb.download((n, m), np.float64), want), (alpha, b is not None, z is not None, gamma)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("cols", [1, 24, 33, 153])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 100, 70001])
def test_transpose_equals_numpy(gpu_ctx, rows, cols):
    a = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) - 7.5
    src, dst = gpu_ctx.buffer(a.nbytes).upload(a), gpu_ctx.buffer(a.nbytes + 8).fill_bytes(0xFF)
    try:
        gpu_ctx.transpose_f64_dev(src.ptr, rows, cols, dst.ptr)
        assert np.array_equal(dst.download((cols, rows), np.float64), a.T)
        assert dst.download((1,), np.int64, a.nbytes)[0] == -1                # nothing written past the end
    finally:
        src.free(), dst.free()


def test_block_calls_check_their_arguments_before_any_launch(gpu_ctx):
    n, m = 5, 3
    indptr, indices, data = _csr(np.random.default_rng(5), n)
    X = np.arange(n * m, dtype=np.float64).reshape(n, m)
    ip, ix, dx, xb, zb = (_up(gpu_ctx, a)[0] for a in (indptr, indices, data, X, X + 1))
    yb = gpu_ctx.buffer(n * m * 8).fill_bytes(0xFF)
    untouched = yb.download((n * m,), np.int64)
    spmm = gpu_ctx.csr_spmm_f64_dev
    try:
        with pytest.raises(ValueError, match="alias"):
            spmm(n, ip.ptr, ix.ptr, dx.ptr, xb.ptr, m, xb.ptr)
        with pytest.raises(ValueError, match="alias"):
            spmm(n, ip.ptr, ix.ptr, dx.ptr, xb.ptr, m, zb.ptr, 1.0, None, zb.ptr, 1.0)
        with pytest.raises(ValueError, match="negative"):
            spmm(-1, ip.ptr, ix.ptr, dx.ptr, xb.ptr, m, yb.ptr)
        with pytest.raises(ValueError, match="negative"):
            spmm(n, ip.ptr, ix.ptr, dx.ptr, xb.ptr, -1, yb.ptr)
        with pytest.raises(ValueError, match="aliased"):
            gpu_ctx.transpose_f64_dev(xb.ptr, n, m, xb.ptr)
        with pytest.raises(ValueError, match="negative"):
            gpu_ctx.transpose_f64_dev(xb.ptr, -1, m, yb.ptr)
        with pytest.raises(ValueError, match="negative"):
            gpu_ctx.transpose_f64_dev(xb.ptr, n, -1, yb.ptr)
        spmm(0, ip.ptr, ix.ptr, dx.ptr, xb.ptr, m, yb.ptr)                     # empty: fine, nothing written
        spmm(n, ip.ptr, ix.ptr, dx.ptr, xb.ptr, 0, yb.ptr)
        gpu_ctx.transpose_f64_dev(xb.ptr, 0, m, yb.ptr)
        gpu_ctx.transpose_f64_dev(xb.ptr, n, 0, yb.ptr)
        assert np.array_equal(yb.download((n * m,), np.int64), untouched)
        assert np.array_equal(xb.download((n, m), np.float64), X)
    finally:
        for b in (ip, ix, dx, xb, zb, yb):
            b.free()


# ================================================================================ the eigensolver against a dense decomposition
TOL = 1e-10            # the residual |S v - theta v| the solver stops at (eigen_tol="auto")


@pytest.mark.parametrize("name", sorted(nc.GRAPHS))
def test_spectral_embedding_equals_the_dense_decomposition(gpu_ctx, name):
    """Eigenvalues within 1e-9 (a Ritz value lies within its residual, at most 1e-10, of an eigenvalue).  Subspace: the maps times
    dd span the top-m eigenvectors of S up to sine <= 2 sqrt(m) tol / gap + 1e-12 -- Davis-Kahan with the residual bound the solver
    stops at (|R|_F <= sqrt(m) tol) and gap = theta_m - theta_{m+1} of the dense reference (>= 1e-3, asserted on the host); the
    factor 2 and the additive term cover the rounding of the two orthonormalisations and of the reference."""
    indptr, indices, N, m = nc.graph(name)
    theta, U, dd = nn.normalised_affinity_eigh(indptr, indices, N)
    max_iter = 500
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        emb, eigs, it = cluster.spectral_embedding(indptr, indices, N, m, random_state=7, max_iter=max_iter, ctx=gpu_ctx)
    messages = [str(w.message) for w in caught]
    connected = nc.GRAPHS[name][2] == 0
    assert [("not fully connected" in s) for s in messages] == ([] if connected else [True]), messages
    assert it < max_iter
    assert emb.shape == (N, m) and eigs.shape == (m,)
    assert np.abs(eigs - (1.0 - theta[:m])).max() <= 1e-9
    gap = theta[m - 1] - theta[m]
    assert gap >= nc.MIN_GAP
    sine = nn.subspace_sine(emb * dd[:, None], U[:, :m])
    assert sine <= 2.0 * np.sqrt(m) * TOL / gap + 1e-12, (sine, gap)
    top = np.abs(emb).argmax(0)
    assert (emb[top, np.arange(m)] > 0).all()                                # the deterministic sign convention
    if not connected:                                                          # isolated nodes carry nothing of the top maps
        assert np.abs(emb[N - nc.GRAPHS[name][2]:]).max() <= 1e-9
