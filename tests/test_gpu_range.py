"""GPU tests of the cosine threshold join and the pair components (csrc/range.hip, pvsim/duplicates.py).  The
yardstick is the full score matrix of the existing Context.cosine_dev on the same device buffers, thresholded in NumPy by the twin
(tests/range_numpy.py); on the lattice it is the twin's exact scores.  Every comparison is on bytes: there is no tolerance here."""
import numpy as np
import pytest

import range_numpy as tw
from test_range_host import BAND, BAND_CAPACITY, LATTICE, LATTICE_T

pytestmark = pytest.mark.gpu

UPPER = 1
GUARD = 8                      # entries behind the capacity that must keep their 0x5A fill


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Rows:
    """float32 rows on the device with their inverse norms (the norm kernel's unless given); `offset` bytes shift the base address"""

    def __init__(self, ctx, x, inv=None, offset=0):
        x = np.ascontiguousarray(x, np.float32)
        self.ctx, self.x, self.n, self.L = ctx, x, x.shape[0], x.shape[1]
        self.buf = ctx.buffer(x.nbytes + offset + 16)
        self.buf.upload(x, offset=offset)
        self.ptr = self.buf.ptr + offset
        self.inv = ctx.buffer(max(self.n * 4, 16))
        if inv is None:
            ctx.row_inv_norms_dev(self.ptr, self.n, self.L, self.inv.ptr)
        else:
            self.inv.upload(np.ascontiguousarray(inv, np.float32))

    def free(self):
        self.buf.free(), self.inv.free()


def _matrix(ctx, q, db):
    """the yardstick: pvs_cosine_dev of the same buffers and norms"""
    out = ctx.buffer(max(q.n * db.n * 4, 16))
    ctx.cosine_dev(q.ptr, q.n, db.ptr, db.n, q.L, q.inv.ptr, db.inv.ptr, out.ptr, db.n)
    S = out.download((q.n, db.n), np.float32)
    out.free()
    return S


def _join(ctx, q, db, t, capacity, flags=0, path=1, tile=0, no_norms=False):
    """-> (row, col, val of the first min(total, capacity) entries, total, stats, over: whether PVS_ERR_CAPACITY came back); the outputs
    are filled with 0x5A first and nothing at or behind the capacity may be written"""
    from pvsim import CapacityError
    n = capacity + GUARD
    outs = [ctx.buffer(n * 8).fill_bytes(0x5A), ctx.buffer(n * 8).fill_bytes(0x5A), ctx.buffer(n * 4).fill_bytes(0x5A)]
    over = False
    try:
        total, stats = ctx.cosine_range_dev(q.ptr, q.n, db.ptr, db.n, q.L, None if no_norms else q.inv.ptr, None if no_norms else db.inv.ptr,
                                            t, capacity, outs[0].ptr, outs[1].ptr, outs[2].ptr, flags=flags, path=path, tile=tile)
    except CapacityError as e:
        total, stats, over = e.args[1], e.args[2], True
    row, col, val = outs[0].download((n,), np.int64), outs[1].download((n,), np.int64), outs[2].download((n,), np.float32)
    m = min(total, capacity)
    for a in (row, col, val):
        assert (a[m:].view(np.uint8) == 0x5A).all(), "written at or beyond min(total, capacity)"
    for b in outs:
        b.free()
    return row[:m], col[:m], val[:m], total, stats, over


def _assert_triples(got, want, where):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), where
    assert np.array_equal(_bits(got[2]), _bits(want[2])), where


def _check_join(ctx, q, db, S, t, *, flags=0, tile=0, paths=(1, 2), expect_filtered=None, where=None):
    """both paths against the twin on S, in the raw device order of the geometry used -> stats of the last path"""
    upper = bool(flags & UPPER)
    QT, NC = (min(q.n, tile), min(db.n, tile)) if tile else (min(q.n, 8192), min(db.n, 32768))
    want = tw.tile_order(S, t, QT, NC, upper)
    for path in paths:
        row, col, val, total, stats, over = _join(ctx, q, db, t, want[0].size, flags=flags, path=path, tile=tile)
        assert total == want[0].size and not over, (where, path, total, want[0].size)
        _assert_triples((row, col, val), want, (where, path))
        if path == 1:
            assert not stats["filtered"] and stats["rescored"] == 0
        elif expect_filtered is not None:
            assert stats["filtered"] == expect_filtered, (where, stats)
        if upper:
            assert stats["tiles_skipped"] == tw.skipped_tiles(q.n, db.n, QT, NC), (where, stats)
    return stats


def _random_rows(rng, n, L):
    x = rng.standard_normal((n, L)).astype(np.float32)
    if n >= 4:
        x[n - 1] = x[0]                      # an exact duplicate: score 1 up to rounding, and equal columns for every query
    return x


# ------------------------------------------------------------------------------------------------ seams
@pytest.mark.parametrize("L", [8, 1032, 2056])              # one, two and three chains of 1024 k
def test_row_and_column_seams(gpu_ctx, L):
    rng = np.random.default_rng(100 + L)
    for N in (1, 63, 64, 65, 129):
        db = _Rows(gpu_ctx, _random_rows(rng, N, L))
        for nq in (1, 3, 4, 5, 65):
            q = _Rows(gpu_ctx, np.concatenate([db.x[:1], _random_rows(rng, nq, L)])[:nq])
            S = _matrix(gpu_ctx, q, db)
            t = np.float32(np.median(S))
            st = _check_join(gpu_ctx, q, db, S, t, expect_filtered=True, where=(L, N, nq))
            assert st["redone_exact"] == 0 and st["tiles"] == 1
            q.free()
        db.free()


@pytest.mark.parametrize("N", [130, 257])
@pytest.mark.parametrize("tile", [64, 128])
def test_tiles_diagonal_and_skipped(gpu_ctx, N, tile):
    rng = np.random.default_rng(N + tile)
    x = _Rows(gpu_ctx, _random_rows(rng, N, 64))
    S = _matrix(gpu_ctx, x, x)
    t = np.float32(np.quantile(S, 0.7))
    st = _check_join(gpu_ctx, x, x, S, t, flags=UPPER, tile=tile, expect_filtered=True, where=("upper", N, tile))
    assert st["tiles_skipped"] > 0 and st["tiles"] + st["tiles_skipped"] == (-(-N // tile)) ** 2
    st = _check_join(gpu_ctx, x, x, S, t, tile=tile, expect_filtered=True, where=("full", N, tile))
    assert st["tiles_skipped"] == 0 and st["tiles"] == (-(-N // tile)) ** 2
    q = _Rows(gpu_ctx, _random_rows(rng, 70, 64))          # rectangular, several tiles on both axes
    S = _matrix(gpu_ctx, q, x)
    _check_join(gpu_ctx, q, x, S, np.float32(0.05), tile=tile // 2, expect_filtered=True, where=("rect", N, tile))
    q.free(), x.free()


def test_rows_that_do_not_qualify_take_the_exact_path(gpu_ctx):
    rng = np.random.default_rng(5)
    for L, offset in ((12, 0), (16, 4), (1032, 4)):          # L % 8 != 0; a base address off the 16-byte grid
        q, db = _Rows(gpu_ctx, _random_rows(rng, 33, L), offset=offset), _Rows(gpu_ctx, _random_rows(rng, 70, L), offset=offset)
        S = _matrix(gpu_ctx, q, db)
        st = _check_join(gpu_ctx, q, db, S, np.float32(0.0), expect_filtered=False, where=(L, offset))
        assert st["rescored"] == 0
        st = _check_join(gpu_ctx, q, db, S, np.float32(0.0), tile=32, expect_filtered=False, where=(L, offset, "tiled"))
        q.free(), db.free()
    q = _Rows(gpu_ctx, _random_rows(rng, 9, 64))               # no norm arrays: raw dot products, and path 2 runs exact
    out = gpu_ctx.buffer(9 * 9 * 4)
    gpu_ctx.cosine_dev(q.ptr, 9, q.ptr, 9, 64, None, None, out.ptr, 9)
    S = out.download((9, 9), np.float32)
    want = tw.hits(S, 1.0)
    for path in (1, 2):
        row, col, val, total, stats, _ = _join(gpu_ctx, q, q, np.float32(1.0), want[0].size, path=path, no_norms=True)
        _assert_triples((row, col, val), want, ("no norms", path))
        assert not stats["filtered"]
    out.free(), q.free()


# ------------------------------------------------------------------------------------------------ threshold
def test_threshold_ties_zero_rows_and_everything(gpu_ctx):
    x = tw.lattice(**LATTICE)
    S = tw.lattice_scores(x, x)                                 # exact: the yardstick on the lattice
    r = _Rows(gpu_ctx, x, inv=tw.lattice_inv(x))
    assert np.array_equal(_bits(_matrix(gpu_ctx, r, r)), _bits(S))
    t = np.float32(LATTICE_T)
    above = np.nextafter(t, np.float32(1))
    ties = int((S == t).sum())
    assert ties > 0
    for tile in (0, 64):
        _check_join(gpu_ctx, r, r, S, t, tile=tile, expect_filtered=True, where=("ties in", tile))
        _check_join(gpu_ctx, r, r, S, above, tile=tile, expect_filtered=True, where=("ties out", tile))
        _check_join(gpu_ctx, r, r, S, t, flags=UPPER, tile=tile, expect_filtered=True, where=("ties upper", tile))
    assert tw.hits(S, t)[0].size - tw.hits(S, above)[0].size == ties
    # the zero row 4 scores 0 against everything: a hit at t = 0 and not above
    row, col, val, total, _, _ = _join(gpu_ctx, r, r, np.float32(0.0), S.size, path=2)
    assert (row == 4).sum() == x.shape[0] and np.array_equal(np.sort(col[row == 4]), np.arange(x.shape[0]))
    row, _, _, _, _, _ = _join(gpu_ctx, r, r, np.nextafter(np.float32(0), np.float32(1)), S.size, path=2)
    assert (row == 4).sum() == 0
    # t = -1 returns all pairs
    for path in (1, 2):
        row, col, val, total, _, over = _join(gpu_ctx, r, r, np.float32(-1.0), S.size, path=path, tile=64)
        assert total == S.size and not over
        _assert_triples((row, col, val), tw.tile_order(S, -1.0, 64, 64), ("all", path))
    r.free()


def test_nan_row_hits_nothing_and_sends_the_prefilter_to_the_exact_path(gpu_ctx):
    rng = np.random.default_rng(9)
    x = _random_rows(rng, 70, 64)
    x[7, 3] = np.nan
    r = _Rows(gpu_ctx, x)
    S = _matrix(gpu_ctx, r, r)
    assert np.isnan(S[7]).all() and np.isnan(S[:, 7]).all()
    for t in (np.float32(-1.0), np.float32(0.1)):
        st = _check_join(gpu_ctx, r, r, S, t, expect_filtered=False, where=("nan", t))
        row, col, _, _, _, _ = _join(gpu_ctx, r, r, t, S.size, path=2)
        assert not (row == 7).any() and not (col == 7).any() and not st["filtered"]
    r.free()


# ------------------------------------------------------------------------------------------------ paths
def test_paths_agree_on_the_band_corpus(gpu_ctx):
    x, place, cos = tw.planted_band(**BAND)
    r = _Rows(gpu_ctx, x)
    S = _matrix(gpu_ctx, r, r)
    t = np.float32(BAND["t"])
    planted = S[place[:, 0], place[:, 1]]
    assert 8 <= (planted >= t).sum() <= len(cos) - 8             # the band straddles the threshold in float32 too
    for tile in (0, 64):
        for flags in (UPPER, 0):
            want = tw.tile_order(S, t, *((tile, tile) if tile else (x.shape[0], x.shape[0])), bool(flags))
            cap = BAND_CAPACITY if flags else 2 * BAND_CAPACITY + x.shape[0]
            got = {}
            for path in (1, 2):
                row, col, val, total, stats, over = _join(gpu_ctx, r, r, t, cap, flags=flags, path=path, tile=tile)
                assert not over and total == want[0].size
                _assert_triples((row, col, val), want, (tile, flags, path))          # the raw device order is the twin's tile order
                order = np.lexsort((col, row))
                got[path] = (row[order], col[order], val[order])
            _assert_triples(got[1], got[2], (tile, flags))
            assert stats["filtered"] and stats["redone_exact"] == 0
            # the prefilter kept more than it returned: the planted pairs just below t were candidates and the exact score refused them
            assert stats["rescored"] >= total + (8 if flags else 16)
    r.free()


def test_staging_overflow_is_redone_by_the_exact_path(gpu_ctx):
    x = _Rows(gpu_ctx, _random_rows(np.random.default_rng(4), 130, 64))
    row, col, val, total, stats, over = _join(gpu_ctx, x, x, np.float32(-1.0), 0, flags=UPPER, path=2, tile=64)
    assert total == 8385 == 130 * 129 // 2 and over and stats["filtered"] and stats["redone_exact"] >= 1
    from pvsim import CapacityError
    with pytest.raises(CapacityError) as e:                      # capacity 0 with NULL outputs: count only
        gpu_ctx.cosine_range_dev(x.ptr, 130, x.ptr, 130, 64, x.inv.ptr, x.inv.ptr, -1.0, 0, None, None, None, flags=UPPER, path=2, tile=64)
    assert e.value.args[1] == 8385
    S = _matrix(gpu_ctx, x, x)                                    # and with room the redone blocks land in order
    want = tw.tile_order(S, -1.0, 64, 64, True)
    row, col, val, total, stats, over = _join(gpu_ctx, x, x, np.float32(-1.0), 1100, flags=UPPER, path=2, tile=64)
    # rows 0..63 bring 63 * 64 / 2 + 64 * 66 = 6240 candidates, the most of any row block: 2 * 1100 + 4096 = 6296 entries hold them
    assert over and total == 8385 and stats["redone_exact"] == 0
    _assert_triples((row, col, val), tuple(a[:1100] for a in want), "first 1100")
    row, col, val, total, stats, over = _join(gpu_ctx, x, x, np.float32(-1.0), 8385, flags=UPPER, path=2, tile=64)
    assert not over
    _assert_triples((row, col, val), want, "all pairs")
    x.free()


# ------------------------------------------------------------------------------------------------ capacity
@pytest.mark.parametrize("path", [1, 2])
def test_capacity_cases(gpu_ctx, path):
    from pvsim import CapacityError
    rng = np.random.default_rng(21)
    q, db = _Rows(gpu_ctx, _random_rows(rng, 37, 64)), _Rows(gpu_ctx, _random_rows(rng, 150, 64))
    S = _matrix(gpu_ctx, q, db)
    t = np.float32(0.15)
    want = tw.tile_order(S, t, 32, 32)
    n = want[0].size
    assert n > 100
    row, col, val, total, _, over = _join(gpu_ctx, q, db, t, n, path=path, tile=32)                 # exact fit
    assert total == n and not over
    _assert_triples((row, col, val), want, "fit")
    row, col, val, total, _, over = _join(gpu_ctx, q, db, t, n - 1, path=path, tile=32)             # one short
    assert total == n and over
    _assert_triples((row, col, val), tuple(a[:n - 1] for a in want), "one short")
    with pytest.raises(CapacityError) as e:                                                          # zero, NULL outputs
        gpu_ctx.cosine_range_dev(q.ptr, q.n, db.ptr, db.n, 64, q.inv.ptr, db.inv.ptr, t, 0, None, None, None, path=path, tile=32)
    assert e.value.args[1] == n
    total, _ = gpu_ctx.cosine_range_dev(q.ptr, q.n, db.ptr, db.n, 64, q.inv.ptr, db.inv.ptr, 2.0, 0, None, None, None, path=path)
    assert total == 0                                                                                # total 0 is no error
    row, col, val, total, _, over = _join(gpu_ctx, q, db, np.float32(2.0), 5, path=path)
    assert total == 0 and not over and row.size == 0
    q.free(), db.free()


def test_arguments_are_checked_before_anything_runs(gpu_ctx):
    x = _Rows(gpu_ctx, _random_rows(np.random.default_rng(2), 8, 16))
    o = gpu_ctx.buffer(1024)
    call = lambda **kw: gpu_ctx.cosine_range_dev(**{**dict(d_q=x.ptr, nq=8, d_db=x.ptr, N=8, L=16, d_invq=x.inv.ptr, d_invdb=x.inv.ptr,
                                                            threshold=0.5, capacity=16, d_row=o.ptr, d_col=o.ptr + 256, d_val=o.ptr + 512), **kw})
    for bad in (dict(threshold=np.nan), dict(threshold=np.inf), dict(flags=UPPER, nq=7), dict(flags=2), dict(path=3), dict(path=-1),
                dict(tile=-1), dict(tile=32769), dict(capacity=-1), dict(capacity=(1 << 40) + 1), dict(d_row=None), dict(d_val=None),
                dict(L=0), dict(d_q=None)):
        with pytest.raises(ValueError):
            call(**bad)
    assert call(nq=0)[0] == 0 and call(N=0)[0] == 0 and call(nq=0, d_q=None)[0] == 0        # no-ops with total 0
    a = gpu_ctx.buffer(64).upload(np.array([0, 1, 8, 2], np.int64))
    with pytest.raises(ValueError):                                                           # node id 8 over 8 nodes
        gpu_ctx.pair_components_dev(a.ptr, a.ptr, 4, 8, o.ptr)
    with pytest.raises(ValueError):
        gpu_ctx.pair_components_dev(a.ptr, a.ptr, 4, 9, None)
    a.free(), o.free(), x.free()


def test_auto_takes_the_prefilter_from_1024_query_rows_on(gpu_ctx):
    """the rule DESIGN.md section 24 derives from profiles/range_timing.jsonl; the triples are the same either way"""
    rng = np.random.default_rng(12)
    db = _Rows(gpu_ctx, _random_rows(rng, 9, 8))
    for nq, filtered in ((1023, False), (1024, True)):
        q = _Rows(gpu_ctx, _random_rows(rng, nq, 8))
        S = _matrix(gpu_ctx, q, db)
        want = tw.hits(S, 0.3)
        row, col, val, total, stats, _ = _join(gpu_ctx, q, db, np.float32(0.3), want[0].size, path=0)
        _assert_triples((row, col, val), want, nq)
        assert stats["filtered"] == filtered
        q.free()
    db.free()


# ------------------------------------------------------------------------------------------------ symmetry
def test_scores_are_symmetric_and_upper_is_half_of_the_full_join(gpu_ctx):
    rng = np.random.default_rng(77)
    x = _random_rows(rng, 130, 1032)
    a, b = _Rows(gpu_ctx, x), _Rows(gpu_ctx, x)                  # the same rows in two buffers: no mirrored symmetric launch
    for path in (1, 2):
        for q, db in ((a, b), (a, a)):
            row, col, val, total, _, _ = _join(gpu_ctx, q, db, np.float32(-1.0), 130 * 130, path=path, tile=64)
            assert total == 130 * 130
            M = np.zeros((130, 130), np.float32)
            M[row, col] = val
            assert np.array_equal(_bits(M), _bits(M.T))           # s(i, j) and s(j, i): the same bits
            t = np.float32(np.quantile(M, 0.6))
            full = _join(gpu_ctx, q, db, t, 130 * 130, path=path, tile=64)
            up = _join(gpu_ctx, q, db, t, 130 * 130, flags=UPPER, path=path, tile=64)
            keep = full[1] > full[0]
            _assert_triples(up[:3], tuple(v[keep] for v in full[:3]), (path, q is db))
    a.free(), b.free()


# ------------------------------------------------------------------------------------------------ components
def _components(ctx, n, a, b):
    a, b = np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64)
    d_a, d_b = ctx.buffer(max(a.nbytes, 16)).upload(a), ctx.buffer(max(b.nbytes, 16)).upload(b)
    d_l = ctx.buffer((n + GUARD) * 4).fill_bytes(0x5A)
    st = ctx.pair_components_dev(d_a.ptr if a.size else None, d_b.ptr if a.size else None, a.size, n, d_l.ptr)
    lab = d_l.download((n + GUARD,), np.int32)
    assert (lab[n:].view(np.uint8) == 0x5A).all()
    for buf in (d_a, d_b, d_l):
        buf.free()
    want = tw.union_find_labels(n, a, b)
    assert np.array_equal(lab[:n], want), (n, a.size)
    assert st["components"] == np.unique(want).size
    assert st["rounds"] <= n + 1 and (st["rounds"] >= 1) == (a.size > 0)
    return st


def test_components_match_the_twin(gpu_ctx):
    rng = np.random.default_rng(8)
    for n in (1, 2, 65, 1000):                                    # path graphs, edges in reverse order
        e = np.arange(n - 1)[::-1]
        st = _components(gpu_ctx, n, e + 1, e)
        # every node k + 1 is hooked by its own edge in the first round (nothing else writes its parent), so the second finds one root
        assert st["components"] == 1 and st["rounds"] == (2 if n > 1 else 0), st
    _components(gpu_ctx, 500, np.full(499, 499), np.arange(499))                          # a star around the LAST node
    n = 301
    ev, od = np.arange(0, n - 2, 2), np.arange(1, n - 2, 2)
    st = _components(gpu_ctx, n, np.concatenate([ev, od]), np.concatenate([ev + 2, od + 2]))      # two interleaved components
    assert st["components"] == 2
    a, b = rng.integers(0, 200, 900), rng.integers(0, 200, 900)
    _components(gpu_ctx, 400, np.concatenate([a, a, b]), np.concatenate([b, b, a]))       # duplicate edges, both directions, isolated nodes 200..
    _components(gpu_ctx, 70, np.arange(5), np.arange(5))                                  # self loops only
    st = _components(gpu_ctx, 129, np.zeros(0, np.int64), np.zeros(0, np.int64))          # E = 0: the identity
    assert st == {"rounds": 0, "components": 129}
    a, b = rng.integers(0, 5000, 3000), rng.integers(0, 5000, 3000)
    _components(gpu_ctx, 5000, a, b)


# ------------------------------------------------------------------------------------------------ Python surface
class _Enc:
    """an encoder whose encoding of an `image` is the image's first row"""
    context = None

    def encode(self, image):
        return np.asarray(image, np.float32).reshape(1, -1)


@pytest.fixture(scope="module")
def corpus(gpu_ctx):
    """a planted corpus: 120 rows of 64 dims in 30 clusters of varying tightness, so a threshold of 0.9 connects some rows and not others"""
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((30, 64))
    x = (centres[rng.integers(0, 30, 120)] + rng.uniform(0.02, 0.5, (120, 1)) * rng.standard_normal((120, 64))).astype(np.float32)
    enc = {f"img_{i:03d}.jpg": x[i] for i in range(120)}
    index = DeviceIndex(enc, gpu_ctx)
    r = _Rows(gpu_ctx, x)
    S = _matrix(gpu_ctx, r, r)
    r.free()
    yield enc, index, x, S
    index.close()


@pytest.mark.parametrize("path", ["auto", "exact", "filtered"])
def test_index_methods_match_the_twin(corpus, path):
    enc, index, x, S = corpus
    t = 0.9
    q = x[[3, 50, 7, 119]]
    indptr, idx, val = index.range_search(q, t, path=path)
    w_ptr, w_idx, w_val = tw.csr(S[[3, 50, 7, 119]], np.float32(t))
    assert np.array_equal(indptr, w_ptr) and np.array_equal(idx, w_idx) and np.array_equal(_bits(val), _bits(w_val))
    assert indptr.dtype == idx.dtype == np.int64 and val.dtype == np.float32 and idx.size >= 4
    assert index.last_range_stats["threshold"] == float(np.float32(t)) and index.last_range_stats["filtered"] == (path == "filtered")
    i, j, s = index.similar_pairs(t, path=path)
    _assert_triples((i, j, s), tw.upper_pairs(S, np.float32(t)), path)
    assert i.size > 20
    e = index.range_search(np.zeros((0, 64), np.float32), t)
    assert e[0].tolist() == [0] and e[1].size == 0 and e[2].size == 0


def test_capacity_retry_and_limits(corpus, gpu_ctx):
    from pvsim import CapacityError
    enc, index, x, S = corpus
    w = tw.csr(S, np.float32(-1.0))
    assert w[1].size == 120 * 120 > max(4096, 4 * 120)            # more than the first call offers: one retry at the reported total
    indptr, idx, val = index.range_search(x, -1.0)
    assert index.last_range_stats["retried"]
    assert np.array_equal(indptr, w[0]) and np.array_equal(idx, w[1]) and np.array_equal(_bits(val), _bits(w[2]))
    i, j, s = index.similar_pairs(-1.0)
    assert index.last_range_stats["retried"] and i.size == 120 * 119 // 2
    index.range_search(x[:2], 0.9)
    assert not index.last_range_stats["retried"]
    n_hit = tw.upper_pairs(S, np.float32(0.9))[0].size
    assert index.similar_pairs(0.9, max_pairs=n_hit)[0].size == n_hit
    for call, total in ((lambda: index.similar_pairs(0.9, max_pairs=n_hit - 1), n_hit),
                        (lambda: index.similar_pairs(-1.0, max_pairs=5000), 120 * 119 // 2),
                        (lambda: index.range_search(x, -1.0, max_results=14399), 14400)):
        with pytest.raises(CapacityError) as e:
            call()
        assert e.value.args[1] == total
    with pytest.raises(ValueError):
        index.range_search(x[:, :32], 0.9)
    with pytest.raises(TypeError):
        index.range_search(x.astype(np.float64), 0.9)


def test_find_duplicates_and_eval_functions(corpus, gpu_ctx):
    import pvsim
    from pvsim import eval as pv_eval
    enc, index, x, S = corpus
    t = 0.9
    pi, pj, ps = tw.upper_pairs(S, np.float32(t))
    labels = tw.union_find_labels(120, pi, pj)
    paths = list(enc)
    for path in ("auto", "filtered"):
        for min_size in (1, 2, 3):
            d = pvsim.find_duplicates(index, t, min_size=min_size, path=path)
            want = tw.groups(labels, min_size)
            assert np.array_equal(d.labels, labels) and d.labels.dtype == np.int64
            assert len(d.groups) == len(want) == len(d) and all(np.array_equal(g, w) for g, w in zip(d.groups, want))
            assert d.paths == [[paths[i] for i in g] for g in want] and list(d) == d.paths
            _assert_triples(d.pairs, (pi, pj, ps), path)
            assert d.stats["pairs"] == pi.size and d.stats["components"] == np.unique(labels).size and d.stats["rounds"] >= 1
            assert d.stats["threshold"] == float(np.float32(t))
    assert 1 < len(tw.groups(labels)) < 60
    want_paths = [[paths[i] for i in g] for g in tw.groups(labels)]
    assert pv_eval.find_duplicates(index, t) == want_paths and pv_eval.find_duplicates(enc, t) == want_paths
    w_ptr, w_idx, w_val = tw.csr(S[[50]], np.float32(t))
    for dataset in (index, enc):
        got = pv_eval.retrieve_similar(x[50][None, :], dataset, _Enc(), t)
        assert [p for p, _ in got] == [paths[i] for i in w_idx] and np.array_equal(_bits([s for _, s in got]), _bits(w_val))
    with pytest.raises(pvsim.CapacityError):
        pv_eval.retrieve_similar(x[50][None, :], index, _Enc(), -1.0, max_results=7)
    none = pvsim.find_duplicates(index, 1.5)
    assert none.groups == [] and np.array_equal(none.labels, np.arange(120)) and none.stats["rounds"] == 0


def test_other_indexes_are_refused_by_name(gpu_ctx):
    import pvsim
    from pvsim import eval as pv_eval
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 64))
    f64 = DeviceIndex({f"p{i}": x[i] for i in range(40)}, gpu_ctx)
    i8 = pvsim.Int8Index({f"p{i}": x[i].astype(np.float32) for i in range(40)}, ctx=gpu_ctx)
    for bad in (f64, i8):
        for call in (lambda: pvsim.find_duplicates(bad, 0.9), lambda: pv_eval.find_duplicates(bad, 0.9),
                     lambda: pv_eval.retrieve_similar(x[:1], bad, _Enc(), 0.9)):
            with pytest.raises(NotImplementedError, match="float32 pvsim.index.DeviceIndex"):
                call()
    for call in (lambda: f64.range_search(x[:2].astype(np.float32), 0.9), lambda: f64.similar_pairs(0.9)):
        with pytest.raises(NotImplementedError, match="float32"):
            call()
    f64.close(), i8.close()
