"""GPU tests of the int8 threshold join (csrc/sq8_range.hip, pvsim/quantized.py).  The yardstick is the NumPy
twin (tests/sq8_range_numpy.py): integer sums and float32 element operations, so every comparison is on bytes and there is no
tolerance here.  Codes and factors go straight to the C entry where a case has to be planted."""
import numpy as np
import pytest

import sq8_numpy as sq
import sq8_range_numpy as tw
from test_sq8_range_host import asymmetric_corpus, random_codes

pytestmark = pytest.mark.gpu

F = np.float32
UPPER = 1
PANEL, MASK = 1, 2
GUARD = 8                      # entries behind the capacity that must keep their 0x5A fill
SIZES = (1, 31, 32, 33, 127, 128, 129, 257)
TILES = (0, 32, 100, 128, 160)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class _Codes:
    """int8 code rows (n, ld) and their factors on the device"""

    def __init__(self, ctx, codes, inv, L):
        self.codes, self.inv_h, self.n, self.L = np.ascontiguousarray(codes, np.int8), np.ascontiguousarray(inv, F), codes.shape[0], L
        assert codes.shape[1] == sq.ld_of(L)
        self.buf = ctx.buffer(max(self.codes.nbytes, 16)).upload(self.codes)
        self.inv = ctx.buffer(max(self.n * 4, 16)).upload(self.inv_h)
        self.ptr = self.buf.ptr

    def free(self):
        self.buf.free(), self.inv.free()


class _Out:
    """the three outputs, filled with 0x5A before every call: nothing at or behind min(total, capacity) may be written"""

    def __init__(self, ctx, entries):
        self.n = entries + GUARD
        self.bufs = [ctx.buffer(self.n * 8), ctx.buffer(self.n * 8), ctx.buffer(self.n * 4)]

    def join(self, ctx, q, db, t, capacity, flags=0, path=MASK, tile=0):
        """-> (row, col, val of the first min(total, capacity) entries, total, stats, over: whether PVS_ERR_CAPACITY came back)"""
        from pvsim import CapacityError
        assert capacity + GUARD <= self.n
        for b in self.bufs:
            b.fill_bytes(0x5A)
        over = False
        try:
            total, stats = ctx.sq8_range_dev(q.ptr, q.inv.ptr, q.n, db.ptr, db.inv.ptr, db.n, q.L, t, capacity, self.bufs[0].ptr,
                                             self.bufs[1].ptr, self.bufs[2].ptr, flags=flags, path=path, tile=tile)
        except CapacityError as e:
            total, stats, over = e.args[1], e.args[2], True
        m = min(total, capacity)
        row, col, val = (self.bufs[0].download((m + GUARD,), np.int64), self.bufs[1].download((m + GUARD,), np.int64),
                         self.bufs[2].download((m + GUARD,), F))
        for a in (row, col, val):
            assert (a[m:].view(np.uint8) == 0x5A).all(), "written at or beyond min(total, capacity)"
        return row[:m], col[:m], val[:m], total, stats, over

    def free(self):
        for b in self.bufs:
            b.free()


def _assert_triples(got, want, where):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), where
    assert np.array_equal(_bits(got[2]), _bits(want[2])), where


def _check(ctx, out, q, db, S, t, *, flags=0, tile=0, paths=(PANEL, MASK), where=None):
    """both paths against the twin on S, each in the raw device order of its own geometry -> stats of the last path"""
    upper = bool(flags & UPPER)
    for path in paths:
        QT, NC = tw.geometry(q.n, db.n, "panel" if path == PANEL else "mask", tile)
        want = tw.rn.tile_order(S, t, QT, NC, upper)
        row, col, val, total, stats, over = out.join(ctx, q, db, t, want[0].size, flags=flags, path=path, tile=tile)
        assert total == want[0].size and not over, (where, path, total, want[0].size)
        _assert_triples((row, col, val), want, (where, path))
        assert (val >= t).all()
        assert stats["path"] == ("panel" if path == PANEL else "mask")
        assert stats["pairs_scored"] == (total if path == MASK else 0)
        skipped = tw.skipped_tiles(q.n, db.n, QT, NC) if upper else 0
        assert stats["tiles_skipped"] == skipped and stats["tiles"] == (-(-q.n // QT)) * (-(-db.n // NC)) - skipped, (where, path, stats)
    return stats


@pytest.fixture(scope="module")
def out(gpu_ctx):
    o = _Out(gpu_ctx, 257 * 257)
    yield o
    o.free()


# ------------------------------------------------------------------------------------------------ shapes, row lengths, tiles
@pytest.mark.parametrize("L", [1, 100, 130, 200])            # ld = 64, 128, 192 (a short last k-block of the GEMM) and 256
def test_every_size_against_every_size(gpu_ctx, out, L):
    """nq, N over the seams of the 32-column word and the 128 x 128 tile; the tile argument cycles with the shape, so that every tile
    size meets every nq and every N"""
    rng = np.random.default_rng(1000 + L)
    dbs = {N: _Codes(gpu_ctx, *random_codes(rng, N, L, zero_rows=(N // 2,) if N > 2 else ()), L) for N in SIZES}
    for a, nq in enumerate(SIZES):
        q = _Codes(gpu_ctx, *random_codes(rng, nq, L), L)
        for b, N in enumerate(SIZES):
            db = dbs[N]
            S = tw.scores(q.codes, q.inv_h, db.codes, db.inv_h)
            t = F(np.quantile(S, 0.8))
            for tile in (TILES[(a + b) % 5], TILES[(a + 2 * b + 1) % 5]):
                _check(gpu_ctx, out, q, db, S, t, tile=tile, where=(L, nq, N, tile))
        q.free()
    for db in dbs.values():
        db.free()


@pytest.mark.parametrize("tile", TILES)
def test_every_tile_size_on_the_largest_shapes(gpu_ctx, out, tile):
    rng = np.random.default_rng(50 + tile)
    for nq, N, L in ((257, 257, 130), (129, 257, 200), (257, 33, 100), (33, 257, 1)):
        q, db = _Codes(gpu_ctx, *random_codes(rng, nq, L), L), _Codes(gpu_ctx, *random_codes(rng, N, L), L)
        S = tw.scores(q.codes, q.inv_h, db.codes, db.inv_h)
        _check(gpu_ctx, out, q, db, S, F(np.quantile(S, 0.7)), tile=tile, where=(nq, N, L, tile))
        q.free(), db.free()


# ------------------------------------------------------------------------------------------------ the self-join
@pytest.mark.parametrize("N", [129, 257])
def test_self_join_diagonal_inside_a_tile_and_tiles_below_it(gpu_ctx, out, N):
    """tile 0: one panel, the diagonal crosses the GEMM's 128-tiles and (N = 257) workgroups lie wholly below it; tiles 100, 128, 160:
    the host skips the panels below the diagonal and the count equals the twin's"""
    rng = np.random.default_rng(N)
    c, inv = random_codes(rng, N, 100, zero_rows=(5,))
    x = _Codes(gpu_ctx, c, inv, 100)
    S = tw.scores(c, inv, c, inv)
    for t in (F(np.quantile(S, 0.6)), F(-2.0)):
        for tile in (0, 32, 100, 128, 160):
            st = _check(gpu_ctx, out, x, x, S, t, flags=UPPER, tile=tile, where=("upper", N, tile))
            if tile and tile < N:
                assert st["tiles_skipped"] > 0
    row, col, val, total, _, _ = out.join(gpu_ctx, x, x, F(-2.0), N * N, flags=UPPER)
    assert total == N * (N - 1) // 2 and (col > row).all()
    x.free()


def test_asymmetric_pairs_are_emitted_as_defined(gpu_ctx, out):
    """s(i, j) < t <= s(j, i) is not emitted, s(j, i) < t <= s(i, j) is: row i < j in the query role decides"""
    c, inv, t = asymmetric_corpus()
    x = _Codes(gpu_ctx, c, inv, 100)
    S = tw.scores(c, inv, c, inv)
    lost, kept = tw.asymmetric_pairs(S, t)
    assert [3, 10] in lost.tolist() and [20, 30] in kept.tolist()
    for path in (PANEL, MASK):
        for tile in (0, 32):
            _check(gpu_ctx, out, x, x, S, t, flags=UPPER, tile=tile, paths=(path,), where=("asymmetric", path, tile))
            row, col, val, _, _, _ = out.join(gpu_ctx, x, x, t, 257 * 257, flags=UPPER, path=path, tile=tile)
            pairs = set(zip(row.tolist(), col.tolist()))
            assert (3, 10) not in pairs and (20, 30) in pairs
            assert not any((a, b) in pairs for a, b in lost.tolist()) and all((a, b) in pairs for a, b in kept.tolist())
            full = out.join(gpu_ctx, x, x, t, 257 * 257, path=path, tile=tile)         # the full join sees both roles
            both = set(zip(full[0].tolist(), full[1].tolist()))
            assert (10, 3) in both and (3, 10) not in both and (20, 30) in both and (30, 20) not in both
    x.free()


# ------------------------------------------------------------------------------------------------ thresholds and capacity
def test_threshold_at_a_score_above_it_below_all_and_above_all(gpu_ctx, out):
    from pvsim import CapacityError
    rng = np.random.default_rng(12)
    qc, iq = random_codes(rng, 129, 130)
    dc, idb = random_codes(rng, 257, 130)
    dc[200] = qc[77]                                                  # a planted pair: the best score of query 77
    idb = sq.factors(dc)
    q, db = _Codes(gpu_ctx, qc, iq, 130), _Codes(gpu_ctx, dc, idb, 130)
    S = tw.scores(qc, iq, dc, idb)
    t = S[77, 200]
    assert t == S[77].max() and t > 0.99
    above = np.nextafter(t, F(2))
    for tile in (0, 100):
        _check(gpu_ctx, out, q, db, S, t, tile=tile, where=("at the score", tile))
        _check(gpu_ctx, out, q, db, S, above, tile=tile, where=("next float above", tile))
    for path in (PANEL, MASK):
        row, col, val, total, _, _ = out.join(gpu_ctx, q, db, t, 100, path=path)
        assert (77, 200) in set(zip(row.tolist(), col.tolist())) and _bits(val[(row == 77) & (col == 200)])[0] == _bits(t)[0]
        row, col, _, _, _, _ = out.join(gpu_ctx, q, db, above, 100, path=path)
        assert (77, 200) not in set(zip(row.tolist(), col.tolist()))
        # below every score: every bit of the mask set; the capacity overflows, the entries below it are written, the retry fits
        low = np.nextafter(S.min(), F(-2))
        want = tw.rn.tile_order(S, low, 100, 100)
        assert want[0].size == 129 * 257
        row, col, val, total, _, over = out.join(gpu_ctx, q, db, low, 1000, path=path, tile=100)
        assert over and total == 129 * 257
        _assert_triples((row, col, val), tuple(a[:1000] for a in want), ("first 1000", path))
        row, col, val, total, _, over = out.join(gpu_ctx, q, db, low, total, path=path, tile=100)
        assert not over and total == 129 * 257
        _assert_triples((row, col, val), want, ("retry", path))
        row, col, val, total, _, over = out.join(gpu_ctx, q, db, low, total - 1, path=path, tile=100)            # one short
        assert over and row.size == total - 1
        # above every score: empty, and no error
        row, _, _, total, st, over = out.join(gpu_ctx, q, db, np.nextafter(S.max(), F(2)), 16, path=path)
        assert total == 0 and not over and row.size == 0 and st["pairs_scored"] == 0
        # capacity 0 with NULL outputs: count only
        n_hit = int((S >= F(0.05)).sum())
        with pytest.raises(CapacityError) as e:
            gpu_ctx.sq8_range_dev(q.ptr, q.inv.ptr, 129, db.ptr, db.inv.ptr, 257, 130, 0.05, 0, None, None, None, path=path)
        assert e.value.args[1] == n_hit > 0
        total, _ = gpu_ctx.sq8_range_dev(q.ptr, q.inv.ptr, 129, db.ptr, db.inv.ptr, 257, 130, 2.0, 0, None, None, None, path=path)
        assert total == 0
    q.free(), db.free()


def test_zero_rows_and_nan_factors(gpu_ctx, out):
    rng = np.random.default_rng(13)
    c, inv = random_codes(rng, 130, 64, zero_rows=(4, 129))
    inv_nan = inv.copy()
    inv_nan[9] = np.nan                                               # a loaded file may hold any factor
    inv_nan[70] = np.inf
    x, y = _Codes(gpu_ctx, c, inv, 64), _Codes(gpu_ctx, c, inv_nan, 64)
    S, Sn = tw.scores(c, inv, c, inv), tw.scores(c, inv_nan, c, inv_nan)
    assert np.isnan(Sn[9, :4]).all() and np.isnan(Sn[4, 70])          # inf * 0
    tiny = np.nextafter(F(0), F(1))
    for tile in (0, 64):
        _check(gpu_ctx, out, x, x, S, F(0.0), tile=tile, where=("zero rows in", tile))
        _check(gpu_ctx, out, x, x, S, tiny, tile=tile, where=("zero rows out", tile))
        _check(gpu_ctx, out, y, y, Sn, F(-10.0), tile=tile, where=("nan", tile))
        _check(gpu_ctx, out, y, y, Sn, F(-10.0), flags=UPPER, tile=tile, where=("nan upper", tile))
    row, col, _, _, _, _ = out.join(gpu_ctx, x, x, F(0.0), 130 * 130)
    assert (row == 4).sum() == 130 and (col == 129).sum() == 130
    row, col, _, _, _, _ = out.join(gpu_ctx, x, x, tiny, 130 * 130)
    assert not (row == 4).any() and not (col == 129).any()
    row, col, _, _, _, _ = out.join(gpu_ctx, y, y, F(-10.0), 130 * 130)
    assert not (row == 9).any() and not (col == 9).any()
    x.free(), y.free()


# ------------------------------------------------------------------------------------------------ paths
def test_panel_path_by_the_row_scan_and_by_the_gemm_and_auto(gpu_ctx, out):
    from pvsim import _ffi
    rng = np.random.default_rng(14)
    db = _Codes(gpu_ctx, *random_codes(rng, 257, 200), 200)
    for nq in (1, 3, 4, 5, 129):
        q = _Codes(gpu_ctx, *random_codes(rng, nq, 200), 200)
        S = tw.scores(q.codes, q.inv_h, db.codes, db.inv_h)
        t = F(np.quantile(S, 0.75))
        for sq8_path in (_ffi.SQ8_PATH_ROWS, _ffi.SQ8_PATH_MATRIX):
            with gpu_ctx.option(_ffi.OPT_SQ8_PATH, sq8_path):
                _check(gpu_ctx, out, q, db, S, t, paths=(PANEL,), where=("sq8 path", sq8_path, nq))
                _check(gpu_ctx, out, q, db, S, t, tile=100, paths=(PANEL,), where=("sq8 path", sq8_path, nq, "tiled"))
                st = out.join(gpu_ctx, q, db, t, 257 * 129, path=0)[4]
                assert st["path"] == ("panel" if sq8_path == _ffi.SQ8_PATH_ROWS else "mask")
        # auto: the panel while the ranking takes the row scan (at most 4 queries), the mask beyond; the triples are the same
        want = tw.rn.tile_order(S, t, nq, 257)
        row, col, val, total, st, _ = out.join(gpu_ctx, q, db, t, want[0].size, path=0)
        _assert_triples((row, col, val), want, ("auto", nq))
        assert st["path"] == ("panel" if nq <= 4 else "mask")
        q.free()
    db.free()


def test_arguments_are_checked_before_anything_runs(gpu_ctx):
    rng = np.random.default_rng(2)
    x = _Codes(gpu_ctx, *random_codes(rng, 8, 16), 16)
    o = gpu_ctx.buffer(1024)
    call = lambda **kw: gpu_ctx.sq8_range_dev(**{**dict(d_qcodes=x.ptr, d_invq=x.inv.ptr, nq=8, d_codes=x.ptr, d_invdb=x.inv.ptr, N=8, L=16,
                                                       threshold=0.5, capacity=16, d_row=o.ptr, d_col=o.ptr + 256, d_val=o.ptr + 512), **kw})
    assert call()[0] >= 0
    for bad in (dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=-np.inf), dict(flags=UPPER, nq=7), dict(flags=2), dict(path=3),
                dict(path=-1), dict(tile=-1), dict(tile=32769), dict(capacity=-1), dict(capacity=(1 << 40) + 1), dict(d_row=None),
                dict(d_col=None), dict(d_val=None), dict(L=0), dict(L=131073), dict(nq=1 << 31), dict(N=1 << 31), dict(d_qcodes=None),
                dict(d_codes=None), dict(d_invq=None), dict(d_invdb=None), dict(d_qcodes=x.ptr + 8), dict(d_codes=x.ptr + 4),
                dict(d_invq=x.inv.ptr + 2), dict(d_row=o.ptr + 4), dict(d_val=o.ptr + 514)):
        with pytest.raises(ValueError):
            call(**bad)
    assert call(nq=0)[0] == 0 and call(N=0)[0] == 0 and call(nq=0, d_qcodes=None, d_invq=None)[0] == 0       # no-ops with total 0
    o.free(), x.free()


def test_poisoned_and_regrown_workspace_gives_the_same_bytes():
    """the one block of WS_PANEL_OUT the entry keeps (panel or mask | counters | row counts | row offsets): a fresh context against one
    whose block was grown by a larger call and filled with 0xFF, 0x00 and 0x5A"""
    import pvsim
    rng = np.random.default_rng(15)
    c, inv = random_codes(rng, 257, 130, zero_rows=(3,))
    big_c, big_inv = random_codes(rng, 600, 130)
    S = tw.scores(c, inv, c, inv)
    t = F(np.quantile(S, 0.9))
    results = {}
    for poisoned in (False, True):
        ctx = pvsim.Context(0)
        try:
            x, o = _Codes(ctx, c, inv, 130), _Out(ctx, 600 * 600)
            for path in (PANEL, MASK):
                for flags, tile in ((0, 0), (UPPER, 100)):
                    fills = (0xFF, 0x00, 0x5A) if poisoned else (None,)
                    for fill in fills:
                        if poisoned:
                            big = _Codes(ctx, big_c, big_inv, 130)
                            o.join(ctx, big, big, F(-2.0), 600 * 600, path=path)         # the block grows beyond what the case needs
                            big.free()
                            assert ctx.diag_ws_bytes()["WS_PANEL_OUT"] > 0
                            ctx.diag_poison(fill)
                        got = o.join(ctx, x, x, t, 257 * 257, flags=flags, path=path, tile=tile)
                        key = (path, flags, tile)
                        if not poisoned:
                            results[key] = got
                            QT, NC = tw.geometry(257, 257, "panel" if path == PANEL else "mask", tile)
                            _assert_triples(got[:3], tw.rn.tile_order(S, t, QT, NC, bool(flags)), key)
                        else:
                            _assert_triples(got[:3], results[key][:3], (key, fill))
                            assert got[3] == results[key][3] and got[4] == results[key][4]
            x.free(), o.free()
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------------ Python surface
@pytest.fixture(scope="module")
def corpus(gpu_ctx):
    """the planted corpus of tests/test_gpu_range.py: 120 rows of 64 dims in 30 clusters of varying tightness"""
    import pvsim
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((30, 64))
    x = (centres[rng.integers(0, 30, 120)] + rng.uniform(0.02, 0.5, (120, 1)) * rng.standard_normal((120, 64))).astype(F)
    enc = {f"img_{i:03d}.jpg": x[i] for i in range(120)}
    index = pvsim.Int8Index(enc, ctx=gpu_ctx)
    codes, inv = sq.encode(x)
    yield enc, index, x, tw.scores(codes, inv, codes, inv)
    index.close()


def _csr_of_rank(index, q, t):
    """rank(k = N) cut at t: the (score descending, index ascending) lists of the ranker, every entry with score >= t"""
    idx, val = index.rank(q, len(index))
    keep = val >= F(t)
    indptr = np.zeros(q.shape[0] + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr, idx[keep], val[keep]


@pytest.mark.parametrize("path", ["auto", "panel", "mask"])
def test_index_methods_match_rank_and_the_twin(corpus, path):
    import pvsim
    enc, index, x, S = corpus
    t = 0.9
    for q in (x[[3, 50, 7, 119]], x[:37] * F(3.0)):                  # 4 queries: the row scan under auto; 37: the GEMM
        indptr, idx, val = index.range_search(q, t, path=path)
        w_ptr, w_idx, w_val = _csr_of_rank(index, q, t)
        assert np.array_equal(indptr, w_ptr) and np.array_equal(idx, w_idx) and np.array_equal(_bits(val), _bits(w_val))
        assert indptr.dtype == idx.dtype == np.int64 and val.dtype == F and idx.size >= 4 and (val >= F(t)).all()
        st = index.last_range_stats
        assert st["threshold"] == float(F(t)) and st["path"] == (path if path != "auto" else ("panel" if len(q) <= 4 else "mask"))
    i, j, s = index.similar_pairs(t, path=path)
    _assert_triples((i, j, s), tw.rn.upper_pairs(S, F(t)), path)
    assert i.size > 20 and index.last_range_stats["path"] == ("mask" if path == "auto" else path)
    ridx, rval = index.rank(x, 120)                                   # every pair's value is what rank of stored row i reports for j
    R = np.zeros((120, 120), F)
    R[np.arange(120)[:, None], ridx] = rval
    assert np.array_equal(_bits(s), _bits(R[i, j])) and (s >= F(t)).all()
    labels = tw.rn.union_find_labels(120, i, j)
    paths = list(enc)
    for min_size in (1, 2, 3):
        d = index.duplicates(t, min_size=min_size, path=path)
        want = tw.rn.groups(labels, min_size)
        assert isinstance(d, pvsim.DuplicateGroups) and np.array_equal(d.labels, labels) and d.labels.dtype == np.int64
        assert len(d.groups) == len(want) and all(np.array_equal(g, w) for g, w in zip(d.groups, want))
        assert d.paths == [[paths[a] for a in g] for g in want]
        _assert_triples(d.pairs, (i, j, s), path)
        assert d.stats["pairs"] == i.size and d.stats["components"] == np.unique(labels).size and d.stats["threshold"] == float(F(t))
    assert 1 < len(tw.rn.groups(labels)) < 60
    e = index.range_search(np.zeros((0, 64), F), t, path=path)
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0


def test_capacity_retry_and_limits(corpus):
    from pvsim import CapacityError
    enc, index, x, S = corpus
    indptr, idx, val = index.range_search(x, -1.0)                     # 14400 > max(4096, 4 * 120): one retry at the reported total
    assert index.last_range_stats["retried"] and idx.size == 120 * 120
    w = _csr_of_rank(index, x, -1.0)
    assert np.array_equal(indptr, w[0]) and np.array_equal(idx, w[1]) and np.array_equal(_bits(val), _bits(w[2]))
    i, j, s = index.similar_pairs(-1.0)
    assert index.last_range_stats["retried"] and i.size == 120 * 119 // 2
    index.range_search(x[:2], 0.9)
    assert not index.last_range_stats["retried"]
    n_hit = tw.rn.upper_pairs(S, F(0.9))[0].size
    assert index.similar_pairs(0.9, max_pairs=n_hit)[0].size == n_hit
    for call, total in ((lambda: index.similar_pairs(0.9, max_pairs=n_hit - 1), n_hit),
                        (lambda: index.similar_pairs(-1.0, max_pairs=5000), 120 * 119 // 2),
                        (lambda: index.range_search(x, -1.0, max_results=14399), 14400)):
        with pytest.raises(CapacityError) as e:
            call()
        assert e.value.args[1] == total


def test_loaded_index_and_index_after_add_and_remove(corpus, gpu_ctx, tmp_path):
    import pvsim
    enc, index, x, S = corpus
    t = 0.9
    index.save(str(tmp_path / "i8"))
    loaded = pvsim.Int8Index.load(str(tmp_path / "i8"), ctx=gpu_ctx)
    for a, b in zip(loaded.similar_pairs(t), index.similar_pairs(t)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for a, b in zip(loaded.range_search(x[:9], t), index.range_search(x[:9], t)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    loaded.close()
    paths = list(enc)
    grown = pvsim.Int8Index({p: enc[p] for p in paths[:70]}, ctx=gpu_ctx)
    grown.add({p: enc[p] for p in paths[70:]})
    gone = [paths[a] for a in (0, 5, 64, 119)]
    grown.remove(gone)
    keep = np.array([a for a in range(120) if paths[a] not in gone])
    codes, inv = sq.encode(x[keep])
    Sk = tw.scores(codes, inv, codes, inv)
    for path in ("panel", "mask"):
        _assert_triples(grown.similar_pairs(t, path=path), tw.rn.upper_pairs(Sk, F(t)), ("updated", path))
        d = grown.duplicates(t, path=path)
        want = tw.rn.union_find_labels(keep.size, *tw.rn.upper_pairs(Sk, F(t))[:2])
        assert np.array_equal(d.labels, want) and d.paths == [[paths[keep[a]] for a in g] for g in tw.rn.groups(want)]
    grown.close()


def test_free_functions_refuse_and_name_the_methods(corpus, gpu_ctx):
    import pvsim
    from pvsim import eval as pv_eval
    enc, index, x, S = corpus
    for call in (lambda: pvsim.find_duplicates(index, 0.9), lambda: pv_eval.find_duplicates(index, 0.9),
                 lambda: pv_eval.retrieve_similar(x[:1], index, None, 0.9)):
        with pytest.raises(NotImplementedError, match="float32 pvsim.index.DeviceIndex") as e:
            call()
        assert all(word in str(e.value) for word in ("Int8Index", "range_search", "similar_pairs", "duplicates"))
    from pvsim.ivf_int8 import IVFInt8Index
    ivf = IVFInt8Index.build(index, x[:4], ctx=gpu_ctx)               # the probed index keeps refusing
    assert not any(hasattr(ivf, m) for m in ("range_search", "similar_pairs", "duplicates"))
    with pytest.raises(NotImplementedError, match="float32 pvsim.index.DeviceIndex") as e:
        pvsim.find_duplicates(ivf, 0.9)
    assert "similar_pairs" not in str(e.value)
    ivf.close()
