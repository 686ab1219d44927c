"""GPU tests of query expansion and database-side augmentation (csrc/expand.hip, pvsim/expand.py, DeviceIndex.rank_expanded /
.augmented, eval's expand=): everything against the NumPy twin (tests/expand_numpy.py), bit for bit -- include/pvsim.h fixes the
order and the rounding of every sum, so there is no tolerance to argue about."""
import ctypes as C

import numpy as np
import pytest

import expand_numpy as tw

pytestmark = pytest.mark.gpu

N_DB = 64
GUARD = 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _up(ctx, a, guard=0):
    """upload; with `guard`, that many 0x5A bytes follow the array"""
    a = np.ascontiguousarray(a)
    b = ctx.buffer(max(a.nbytes + guard, 16))
    if guard:
        b.fill_bytes(0x5A)
    if a.size:
        b.upload(a)
    return b


def _guard_intact(buf, nbytes):
    return (buf.download((GUARD,), np.uint8, offset=nbytes) == 0x5A).all()


def _database(rng, dtype, L):
    """rows whose magnitudes span 2^-12 .. 2^12: sums of them depend on the order of the adds"""
    return (rng.standard_normal((N_DB, L)) * np.exp2(rng.integers(-12, 13, (N_DB, 1)))).astype(dtype)


def _lists(rng, dtype, n, r):
    """idx with -1 slots, slots >= N, a repeated index and (from two rows up) one row with every slot skipped; weights over
    2^-20 .. 2^20 with negative and zero ones"""
    idx = rng.integers(0, N_DB, (n, r)).astype(np.int64)
    w = (rng.standard_normal((n, r)) * np.exp2(rng.integers(-20, 21, (n, r)))).astype(dtype)
    if r:
        w[rng.random((n, r)) < 0.1] = 0
        skip = rng.random((n, r)) < 0.15
        idx[skip] = rng.choice(np.array([-1, -7, N_DB, N_DB + 5, 1 << 40, -(1 << 40)]), int(skip.sum()))
        if r >= 2:
            idx[:, r - 1] = idx[:, 0]                       # a repeated index (or a repeated skip)
        if n >= 2:
            idx[1] = np.where(np.arange(r) % 2 == 0, -1, N_DB)     # nothing of this row's list counts
    return idx, w


def _run_combine(ctx, d_x, X, idx, w, selfr, w_self, in_place):
    """one call -> (output rows, guard intact)"""
    n, r = idx.shape
    L = X.shape[1]
    dt = X.dtype
    d_idx, d_w = _up(ctx, idx), _up(ctx, w)
    d_self = _up(ctx, selfr, GUARD) if selfr is not None else None
    d_ws = _up(ctx, w_self) if w_self is not None else None
    d_out = d_self if in_place else _up(ctx, np.full((n, L), np.nan, dt), GUARD)
    ctx.combine_rows_dev(d_x.ptr, N_DB, L, dt == np.float64, d_self.ptr if d_self else None, d_ws.ptr if d_ws else None,
                         d_idx.ptr if r else None, d_w.ptr if r else None, n, r, d_out.ptr)
    got = d_out.download((n, L), dt)
    ok = _guard_intact(d_out, n * L * dt.itemsize)
    for b in (d_idx, d_w, d_self, d_ws, None if in_place else d_out):
        if b is not None:
            b.free()
    return got, ok


def _row_lengths(ctx, dtype):
    chunk = ctx.COMBINE_CHUNK_BYTES // np.dtype(dtype).itemsize
    return [1, 3, 4, 255, 256, 257, chunk - 1, chunk, chunk + 4, 32768]


def _list_lengths(ctx):
    u = ctx.COMBINE_BATCH
    return [0, 1, 2, u - 1, u, u + 1, 33]


MODES = ("no self", "self and w_self", "self, w_self NULL", "out is self")


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("li", range(10))
def test_combine_matches_twin(gpu_ctx, dtype, li):
    L = _row_lengths(gpu_ctx, dtype)[li]
    rng = np.random.default_rng(1000 + 17 * li + (dtype == np.float64))
    X = _database(rng, dtype, L)
    d_x = _up(gpu_ctx, X)
    case = 0
    for r in _list_lengths(gpu_ctx):
        for n in (1, 5, 300):
            if L == 32768 and n == 300 and r not in (1, gpu_ctx.COMBINE_BATCH + 1):
                continue            # 16 chunks x 300 rows with a short and a batched list; the other list lengths are crossed with n = 300 at every shorter L
            idx, w = _lists(rng, dtype, n, r)
            selfr = _database(rng, dtype, L)[rng.integers(0, N_DB, n)]
            w_self = (rng.standard_normal(n) * np.exp2(rng.integers(-4, 5, n))).astype(dtype)
            if r >= gpu_ctx.COMBINE_BATCH - 1 and n == (5 if L >= 256 else 300):
                # the inputs can tell a reordered sum from the defined one: the twin with j descending gives other bits
                assert not np.array_equal(_bits(tw.combine(X, idx, w, selfr, w_self)), _bits(tw.combine(X, idx, w, selfr, w_self, reverse=True)))
            modes = range(4) if L < 32768 else [case % 4]          # the long rows take the four variants in turn
            for mode in modes:
                s = None if mode == 0 else selfr
                ws = w_self if mode in (1, 3) else None
                got, guard_ok = _run_combine(gpu_ctx, d_x, X, idx, w, s, ws, in_place=mode == 3)
                want = tw.combine(X, idx, w, s, ws)
                assert np.array_equal(_bits(got), _bits(want)), (dtype.__name__, L, r, n, MODES[mode])
                assert guard_ok, (dtype.__name__, L, r, n, MODES[mode])
                if n >= 2 and mode == 0:
                    assert not got[1].any() and not np.signbit(got[1]).any()         # every slot skipped: +0
            case += 1
    d_x.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_combine_unaligned_matrices(gpu_ctx, dtype):
    """rows of a 16-byte multiple that do not START on 16-byte boundaries take the element-wise path"""
    rng = np.random.default_rng(77)
    L, n, r = 260, 9, 11
    isz = np.dtype(dtype).itemsize
    X = _database(rng, dtype, L)
    idx, w = _lists(rng, dtype, n, r)
    selfr = _database(rng, dtype, L)[:n]
    pad = np.zeros(1, dtype)
    d_x = _up(gpu_ctx, np.concatenate([pad, X.ravel()]))
    d_self = _up(gpu_ctx, np.concatenate([pad, selfr.ravel()]))
    d_idx, d_w = _up(gpu_ctx, idx), _up(gpu_ctx, w)
    d_out = gpu_ctx.buffer(isz + n * L * isz + GUARD).fill_bytes(0x5A)
    want = tw.combine(X, idx, w, selfr, None)
    for x_off, s_off, o_off in ((isz, 0, 0), (0, isz, 0), (0, 0, isz), (isz, isz, isz)):
        x = d_x.ptr + x_off if x_off else None
        if x is None:                                        # an aligned copy of X for this variant
            d_xa = _up(gpu_ctx, X)
            x = d_xa.ptr
        s = d_self.ptr + s_off if s_off else None
        if s is None:
            d_sa = _up(gpu_ctx, selfr)
            s = d_sa.ptr
        gpu_ctx.combine_rows_dev(x, N_DB, L, dtype == np.float64, s, None, d_idx.ptr, d_w.ptr, n, r, d_out.ptr + o_off)
        got = d_out.download((n, L), dtype, offset=o_off)
        assert np.array_equal(_bits(got), _bits(want)), (x_off, s_off, o_off)
        assert (d_out.download((GUARD - isz,), np.uint8, offset=o_off + n * L * isz) == 0x5A).all()


def test_combine_no_rows_is_a_no_op(gpu_ctx):
    for f64 in (False, True):
        gpu_ctx.combine_rows_dev(None, 0, 8, f64, None, None, None, None, 0, 3, None)
        gpu_ctx.combine_rows_dev(None, 64, 8, f64, None, None, None, None, 0, 0, None)


def test_combine_refuses_bad_arguments(gpu_ctx):
    """PVS_ERR_INVALID for every bad call, decided on the host: the output (and its guard) keeps its fill"""
    from pvsim import _ffi
    lib = _ffi.lib()
    rng = np.random.default_rng(3)
    L, n, r, isz = 8, 4, 3, 4
    X = _database(rng, np.float32, L)
    idx, w = rng.integers(0, N_DB, (n, r)).astype(np.int64), np.ones((n, r), np.float32)
    d_x, d_idx, d_w = _up(gpu_ctx, X), _up(gpu_ctx, idx), _up(gpu_ctx, w)
    d_self = _up(gpu_ctx, np.ones((2 * n, L), np.float32))
    d_out = gpu_ctx.buffer(n * L * isz + GUARD).fill_bytes(0x5A)

    def call(x=d_x.ptr, N=N_DB, L=L, f64=0, s=None, ws=None, i=d_idx.ptr, ww=d_w.ptr, n=n, r=r, o=d_out.ptr):
        p = lambda v: C.c_void_p(v)
        return lib.pvs_combine_rows_dev(gpu_ctx.handle, p(x), N, L, f64, p(s), p(ws), p(i), p(ww), n, r, p(o))

    xbytes = N_DB * L * isz
    bad = {
        "out is X": dict(o=d_x.ptr),
        "out starts inside X": dict(o=d_x.ptr + xbytes - 16),
        "out ends inside X": dict(x=d_out.ptr + 16, N=2),
        "out covers X": dict(x=d_out.ptr + 32, N=1),
        "L = 0": dict(L=0), "L < 0": dict(L=-4), "N < 0": dict(N=-1), "r < 0": dict(r=-1), "n < 0": dict(n=-1),
        "n < 0 with no pointers": dict(n=-1, x=None, i=None, ww=None, o=None),
        "null out": dict(o=None), "null idx": dict(i=None), "null w": dict(ww=None), "null X": dict(x=None),
        "out overlaps self, shifted": dict(s=d_self.ptr, o=d_self.ptr + L * isz),
        "float64 rows at a 4-byte address": dict(f64=1, o=d_out.ptr + 4, N=8, n=1),
    }
    for what, kw in bad.items():
        assert call(**kw) == _ffi.PVS_ERR_INVALID, what
        assert lib.pvs_last_error()
    with pytest.raises(ValueError):
        gpu_ctx.combine_rows_dev(d_x.ptr, N_DB, 0, False, None, None, d_idx.ptr, d_w.ptr, n, r, d_out.ptr)
    gpu_ctx.sync()
    assert (d_out.download((n * L * isz + GUARD,), np.uint8) == 0x5A).all()
    assert (d_self.download((2 * n, L), np.float32) == 1).all()
    # what is allowed: out directly behind X, out == self, no X needed without lists or without database rows
    after = gpu_ctx.buffer(xbytes + n * L * isz)
    after.upload(X)
    assert call(x=after.ptr, o=after.ptr + xbytes) == _ffi.PVS_OK
    assert call(s=d_self.ptr, o=d_self.ptr) == _ffi.PVS_OK
    assert call(x=None, r=0, i=None, ww=None) == _ffi.PVS_OK
    assert call(x=None, N=0) == _ffi.PVS_OK
    gpu_ctx.sync()
    assert np.array_equal(_bits(after.download((n, L), np.float32, offset=xbytes)), _bits(tw.combine(X, idx, w)))
    assert not d_out.download((n, L), np.float32).any()                      # N = 0: every slot skipped


# ------------------------------------------------------------------------------------------------ rank_expanded
def _corpus(seed, N, L, dtype, classes=12):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((classes, L))
    lab = rng.integers(0, classes, N)
    return (centres[lab] + 0.7 * rng.standard_normal((N, L))).astype(dtype), lab, centres


@pytest.fixture(scope="module")
def indexes(gpu_ctx):
    """one float32 and one float64 index over N = 300 rows of L = 96, their queries, and the queries' device norms"""
    from pvsim.index import DeviceIndex
    out = {}
    for dtype in (np.float32, np.float64):
        X, lab, centres = _corpus(21, 300, 96, dtype)
        rng = np.random.default_rng(22)
        ql = rng.integers(0, len(centres), 7)
        Q = (centres[ql] + 0.9 * rng.standard_normal((7, 96))).astype(dtype)
        index = DeviceIndex({f"img/{i:04d}.jpg": X[i] for i in range(len(X))}, gpu_ctx)
        qindex = DeviceIndex({str(i): Q[i] for i in range(len(Q))}, gpu_ctx)
        out[dtype] = (index, X, Q, qindex.inv_norms.copy())
        qindex.close()
    yield out
    for index, *_ in out.values():
        index.close()


def _members(rng, nq, m, N):
    mem = np.stack([rng.choice(N, m, replace=False) for _ in range(nq)]).astype(np.int64)
    mem[rng.random((nq, m)) < 0.3] = -1
    mem[0] = -1                                                # a query with no member at all: it stays the query
    return mem


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("scheme", ["average", "alpha", "linear"])
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("with_members", [False, True])
def test_rank_expanded_matches_twin(indexes, dtype, scheme, passes, with_members):
    from pvsim import QueryExpansion
    index, X, Q, inv_q = indexes[dtype]
    N, k = len(X), 9
    qe = QueryExpansion(n=6, scheme=scheme, alpha=3, query_weight=0.75, passes=passes)
    inv_db = index.inv_norms
    assert inv_db.dtype == dtype and inv_db.shape == (N,) and index.inv_norms is inv_db         # downloaded once
    if with_members:
        idx = _members(np.random.default_rng(31), len(Q), qe.n, N)
        full_i, full_v = index.rank(Q, N)
        scores = np.empty((len(Q), N), dtype)
        np.put_along_axis(scores, full_i, full_v, axis=1)
        val = np.take_along_axis(scores, np.where(idx >= 0, idx, 0), axis=1)
        got_i, got_v, got_q = index.rank_expanded(Q, k, qe, members=idx, return_queries=True)
    else:
        idx, val = index.rank(Q, qe.n)
        got_i, got_v, got_q = index.rank_expanded(Q, k, qe, return_queries=True)
    rows = tw.expand_queries(Q, inv_q, X, inv_db, idx, val, scheme, 3, 0.75)
    for _ in range(passes - 1):
        idx, val = index.rank(rows, qe.n)
        rows = tw.expand_queries(Q, inv_q, X, inv_db, idx, val, scheme, 3, 0.75)
    assert got_q.dtype == dtype and np.array_equal(_bits(got_q), _bits(rows))
    want_i, want_v = index.rank(rows, k)
    assert np.array_equal(got_i, want_i) and np.array_equal(_bits(got_v), _bits(want_v))
    two = index.rank_expanded(Q, k, qe, members=idx if with_members and passes == 1 else None)
    assert len(two) == 2
    if not with_members:
        assert np.array_equal(two[0], got_i) and np.array_equal(_bits(two[1]), _bits(got_v))
    if with_members and passes == 1:
        assert np.array_equal(_bits(got_q[0]), _bits(dtype(0.75) * inv_q[0] * Q[0] + np.zeros(96, dtype)))   # no member: the scaled query


def test_rank_expanded_arguments(indexes):
    from pvsim import QueryExpansion
    index, X, Q, _ = indexes[np.float32]
    qe = QueryExpansion(n=4)
    with pytest.raises(TypeError):
        index.rank_expanded(Q.astype(np.float64), 5, qe)            # a float64 query against a float32 index
    with pytest.raises(TypeError):
        index.rank_expanded(Q, 5, {"n": 4})
    with pytest.raises(ValueError):
        index.rank_expanded(Q[:, :50], 5, qe)
    with pytest.raises(ValueError):
        index.rank_expanded(Q, 0, qe)
    with pytest.raises(ValueError):
        index.rank_expanded(Q, 5, qe, members=np.full((len(Q), 4), len(X)))
    with pytest.raises(ValueError):
        index.rank_expanded(Q, 5, qe, members=np.zeros((len(Q) + 1, 4), np.int64))
    i, v = index.rank_expanded(Q[:0], 5, qe)
    assert i.shape == (0, 5) and v.shape == (0, 5)
    index64 = indexes[np.float64][0]
    i32, v32 = index64.rank_expanded(Q, 5, qe)                      # float32 queries against a float64 index: ranked in float64
    i64, v64 = index64.rank_expanded(Q.astype(np.float64), 5, qe)
    assert v32.dtype == np.float64 and np.array_equal(i32, i64) and np.array_equal(v32, v64)
    big = QueryExpansion(n=1000)                                    # n beyond N: the whole database is the list
    i, v = index.rank_expanded(Q, 5, big)
    idx, val = index.rank(Q, len(X))
    rows = tw.expand_queries(Q, indexes[np.float32][3], X, index.inv_norms, idx, val, "average", 3, 1.0)
    assert np.array_equal(i, index.rank(rows, 5)[0])


# ------------------------------------------------------------------------------------------------ augmented
def _check_augmented(gpu_ctx, X, r, scheme, block):
    from pvsim.index import DeviceIndex
    N, L = X.shape
    paths = [f"db/{i:05d}.png" for i in range(N)]
    index = DeviceIndex(dict(zip(paths, X)), gpu_ctx)
    before = index.rank(X[:3], min(N, 4))
    aug = index.augmented(r=r, scheme=scheme, alpha=2, block=block)
    kk = min(r, N - 1) + 1
    lists = [index.rank(X[b0:b0 + block], kk) for b0 in range(0, N, block)]          # the device's own lists, block by block
    idx, val = np.concatenate([p[0] for p in lists]), np.concatenate([p[1] for p in lists])
    want = tw.augment(X, index.inv_norms, idx, val, scheme, 2)
    assert aug.matrix.dtype == X.dtype and np.array_equal(_bits(aug.matrix), _bits(want))
    assert list(aug) == paths and list(index) == paths and aug is not index
    assert np.array_equal(_bits(aug[paths[N - 1]]), _bits(want[N - 1]))
    assert np.array_equal(_bits(index.matrix), _bits(X))                            # the source index is untouched, host and device
    after = index.rank(X[:3], min(N, 4))
    assert np.array_equal(before[0], after[0]) and np.array_equal(_bits(before[1]), _bits(after[1]))
    fresh = DeviceIndex(dict(zip(paths, want)), gpu_ctx)                            # the new index ranks like one built from its rows
    assert np.array_equal(_bits(aug.inv_norms), _bits(fresh.inv_norms))
    a, b = aug.rank(X[:5], min(N, 3)), fresh.rank(X[:5], min(N, 3))
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    for ix in (index, aug, fresh):
        ix.close()
    return idx, want


@pytest.mark.parametrize("N,block,dtype,scheme", [(300, 4096, np.float32, "linear"), (300, 4096, np.float64, "alpha"),
                                                  (700, 256, np.float32, "alpha"), (700, 600, np.float32, "linear"),
                                                  (300, 100, np.float64, "average")])
def test_augmented_matches_twin(gpu_ctx, N, block, dtype, scheme):
    X, _, _ = _corpus(40 + N, N, 96, dtype)
    X[N - 20] = X[4]                                           # one exact duplicate pair
    idx, _ = _check_augmented(gpu_ctx, X, 10, scheme, block)
    assert idx.shape == (N, 11)
    assert 4 in idx[N - 20] and N - 20 in idx[4]


def test_augmented_without_self_in_the_list(gpu_ctx):
    """four identical rows and r = 2: the last of them does not find itself among its three best -- the last slot goes"""
    X, _, _ = _corpus(50, 300, 96, np.float32)
    X[[40, 90, 200]] = X[7]
    idx, _ = _check_augmented(gpu_ctx, X, 2, "linear", 4096)
    assert 200 not in idx[200] and 7 in idx[7]


def test_augmented_tiny_indexes(gpu_ctx):
    X, _, _ = _corpus(60, 5, 96, np.float32)
    idx, _ = _check_augmented(gpu_ctx, X, 10, "linear", 4096)       # r beyond N - 1: every other row
    assert idx.shape == (5, 5)
    one = X[:1]
    idx, want = _check_augmented(gpu_ctx, one, 10, "linear", 4096)  # N = 1: the row times its inverse norm
    assert idx.shape == (1, 1)
    from pvsim.index import DeviceIndex
    index = DeviceIndex({"a": one[0]}, gpu_ctx)
    assert np.array_equal(_bits(want), _bits(np.zeros_like(one) + index.inv_norms[:, None] * one))
    for bad in (dict(r=0), dict(block=0), dict(scheme="mean"), dict(alpha=9)):
        with pytest.raises(ValueError):
            index.augmented(**bad)
    index.close()


def test_expansion_helps_on_the_planted_corpus(gpu_ctx):
    """the planted corpus of tests/test_expand_host.py on the device: precision@20 after AQE (n = 5) and after DBA (r = 8, linear)
    each beat the plain ranking by at least 0.05"""
    from pvsim import QueryExpansion
    from pvsim.index import DeviceIndex
    X, lab, Q, ql = tw.planted(seed=0)
    index = DeviceIndex({str(i): X[i] for i in range(len(X))}, gpu_ctx)
    base = tw.precision(index.rank(Q, 20)[0], lab, ql)
    aqe = tw.precision(index.rank_expanded(Q, 20, QueryExpansion(n=5))[0], lab, ql)
    aug = index.augmented(r=8, scheme="linear")
    dba = tw.precision(aug.rank(Q, 20)[0], lab, ql)
    print(f"precision@20: plain {base:.4f}, AQE(n=5) {aqe:.4f}, DBA(r=8, linear) {dba:.4f}")
    index.close(), aug.close()
    assert aqe >= base + 0.05
    assert dba >= base + 0.05


# ------------------------------------------------------------------------------------------------ pvsim.eval
class StubEncoder:
    """an "image" is a (2, 2, 3) uint8 array filled with the number of its query row"""

    def __init__(self, rows, ctx):
        self.rows, self.context = rows, ctx

    def encode(self, images):
        if isinstance(images, list):
            return np.stack([self.rows[int(im[0, 0, 0])] for im in images])
        return self.rows[int(images[0, 0, 0])]


def _image(i):
    return np.full((2, 2, 3), i, np.uint8)


def _average_precision(row, db_labels, true_label):
    hits, total = 0, 0.0
    for rank, i in enumerate(row, start=1):
        if db_labels[i] == true_label:
            hits += 1
            total += hits / rank
    return total / hits if hits else 0.0


def test_eval_with_expansion(gpu_ctx, indexes):
    from pvsim import QueryExpansion
    from pvsim import eval as ev
    index, X, Q, _ = indexes[np.float32]
    paths = list(index)
    as_dict = {p: X[i] for i, p in enumerate(paths)}
    enc = StubEncoder(Q, gpu_ctx)
    qe = QueryExpansion(n=5, scheme="alpha", alpha=2)
    idx, val = index.rank_expanded(Q, 6, qe)
    for i in (0, 3):
        want = [(paths[c], s) for c, s in zip(idx[i], val[i])]
        assert ev.retrieve_top_k_similar(_image(i), index, enc, k=6, expand=qe) == want
        assert ev.retrieve_top_k_similar(_image(i), as_dict, enc, k=6, expand=qe) == want
    # expand=None: today's results
    pi, pv = index.rank(Q, 6)
    plain = [(paths[c], s) for c, s in zip(pi[2], pv[2])]
    assert ev.retrieve_top_k_similar(_image(2), index, enc, k=6) == plain
    assert ev.retrieve_top_k_similar(_image(2), index, enc, k=6, expand=None) == plain
    assert ev.retrieve_top_k_similar(_image(2), as_dict, enc, k=6, expand=None) == plain
    # the metrics over the expanded lists
    labels = {p: i % 12 for i, p in enumerate(paths)}
    db_labels = [labels[p] for p in paths]
    qlab = [int(db_labels[c]) for c in pi[:, 0]]
    images = [_image(i) for i in range(len(Q))]
    want_map = float(np.mean([_average_precision(row, db_labels, t) for row, t in zip(idx, qlab)]))
    want_acc = sum(any(db_labels[c] == t for c in row) for row, t in zip(idx, qlab)) / len(Q)
    for data in (index, as_dict):
        assert ev.top_k_map(images, qlab, data, labels, enc, k=6, expand=qe) == want_map
        assert ev.top_k_accuracy(images, qlab, data, labels, enc, k=6, expand=qe) == want_acc
    assert ev.top_k_map(images, qlab, index, labels, enc, k=6) == ev.top_k_map(images, qlab, as_dict, labels, enc, k=6, expand=None)
    full_i, _ = index.rank_expanded(Q, len(X), qe)                  # k=None: the complete expanded ranking
    assert ev.top_k_map(images, qlab, index, labels, enc, expand=qe) == float(
        np.mean([_average_precision(row, db_labels, t) for row, t in zip(full_i, qlab)]))


def test_expand_verified(gpu_ctx, indexes):
    from pvsim import QueryExpansion
    from pvsim import eval as ev
    index, X, Q, inv_q = indexes[np.float32]
    paths = list(index)
    as_dict = {p: X[i] for i, p in enumerate(paths)}
    enc = StubEncoder(Q, gpu_ctx)
    # what rerank_spatial returns: (path, similarity, inliers); verified = at least 4 inliers, the first qe.n of them
    ranked = [(paths[30], 0.9, 12), (paths[7], 0.8, 3), (paths[99], 0.7, 4), (paths[5], 0.6, 0), (paths[250], 0.5, 9), (paths[2], 0.4, 1)]
    qe = QueryExpansion(n=2, scheme="alpha", alpha=3)
    members = np.array([[30, 99]], np.int64)
    wi, wv, wq = index.rank_expanded(Q[1:2], 4, qe, members=members, return_queries=True)
    want = [(paths[c], s) for c, s in zip(wi[0], wv[0])]
    assert ev.expand_verified(_image(1), ranked, index, enc, k=4, qe=qe) == want
    assert ev.expand_verified(_image(1), ranked, as_dict, enc, k=4, qe=qe) == want
    full_i, full_v = index.rank(Q[1:2], len(X))
    val = np.array([[full_v[0][list(full_i[0]).index(30)], full_v[0][list(full_i[0]).index(99)]]], np.float32)
    rows = tw.expand_queries(Q[1:2], inv_q[1:2], X, index.inv_norms, members, val, "alpha", 3, 1.0)
    assert np.array_equal(_bits(wq), _bits(rows))                    # exactly the verified members, and nothing else
    # a list longer than the verified entries is padded with empty slots; min_inliers moves the bar
    three = ev.expand_verified(_image(1), ranked, index, enc, k=4, qe=QueryExpansion(n=5), min_inliers=4)
    wi3, wv3 = index.rank_expanded(Q[1:2], 4, QueryExpansion(n=5), members=np.array([[30, 99, 250, -1, -1]]))
    assert three == [(paths[c], s) for c, s in zip(wi3[0], wv3[0])]
    high = ev.expand_verified(_image(1), ranked, index, enc, k=4, qe=QueryExpansion(n=5), min_inliers=10)
    wi1, wv1 = index.rank_expanded(Q[1:2], 4, QueryExpansion(n=5), members=np.array([[30, -1, -1, -1, -1]]))
    assert high == [(paths[c], s) for c, s in zip(wi1[0], wv1[0])]
    # nothing verified: the incoming order, without the inlier counts
    assert ev.expand_verified(_image(1), ranked, index, enc, k=4, qe=qe, min_inliers=13) == [(p, s) for p, s, _ in ranked[:4]]
    assert ev.expand_verified(_image(1), [], index, enc, k=4) == []
    # the default: average expansion over 10
    dflt = ev.expand_verified(_image(1), ranked, index, enc, k=3)
    wi0, wv0 = index.rank_expanded(Q[1:2], 3, QueryExpansion(), members=np.array([[30, 99, 250] + [-1] * 7]))
    assert dflt == [(paths[c], s) for c, s in zip(wi0[0], wv0[0])]
