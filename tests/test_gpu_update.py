"""Index maintenance on the GPU: the kernels of csrc/update.hip against the NumPy twin (tests/update_numpy.py)
at the scan's tile seams, every move width and alignment, window seams of the in-place compaction and every list state; then
DeviceIndex, CompactIndex and IVFCompactIndex after adds and removes against an index constructed from the surviving rows through the
same public pieces.  Every comparison is np.array_equal, on bit patterns where the values are floats."""
import numpy as np
import pytest

import update_numpy as up

pytestmark = pytest.mark.gpu

GUARD = 64          # bytes behind a device array that must stay as they were


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _up(ctx, a, extra=0, offset=0, fill=0xA5):
    """device buffer holding `a` at byte `offset`, `extra` bytes of `fill` behind it"""
    a = np.ascontiguousarray(a)
    buf = ctx.buffer(max(offset + a.nbytes + extra, 16))
    buf.fill_bytes(fill)
    if a.nbytes:
        buf.upload(a, offset=offset)
    return buf


def _masks(n, T):
    out = {"all kept": np.ones(n, np.uint8), "none kept": np.zeros(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8)}
    if n:
        for name, i in (("first removed", 0), ("last removed", n - 1)):
            k = np.ones(n, np.uint8)
            k[i] = 0
            out[name] = k
    if n > T + 3:
        k = np.ones(n, np.uint8)
        k[T - 3:T + 3] = 0
        out["run over a tile seam"] = k
    out["random bytes"] = (np.random.default_rng(n).integers(0, 4, n) * 85).astype(np.uint8)[:n] & np.uint8(0xF0)
    return out


def _positions(ctx, keep):
    n = keep.size
    d_keep, d_pos = _up(ctx, keep), _up(ctx, np.full(n + 1, -7, np.int64), GUARD)
    ctx.keep_positions_dev(d_keep.ptr, n, d_pos.ptr)
    pos, guard = d_pos.download((n + 1,), np.int64), d_pos.download((GUARD,), np.uint8, offset=(n + 1) * 8)
    d_keep.free(), d_pos.free()
    assert (guard == 0xA5).all()
    return pos


# ------------------------------------------------------------------------------------------------ keep mask, keep positions
def test_scan_at_its_seams(gpu_ctx):
    T = gpu_ctx.SCAN_TILE
    assert T == up.SCAN_TILE
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 5, T * T + 1):        # T^2 + 1 flags: the third level has two entries
        for name, keep in _masks(n, T).items():
            if n > 4 * T and name not in ("alternating", "last removed", "random bytes"):
                continue                                            # the large size is there for the upper levels; the patterns ran below
            assert np.array_equal(_positions(gpu_ctx, keep), up.keep_positions(keep)), (n, name)
    keep = np.ones(T * T + 1, np.uint8)                             # a removed run over the seam between two second-level blocks
    keep[T * T - 5:] = 0
    assert np.array_equal(_positions(gpu_ctx, keep), up.keep_positions(keep))


def test_scan_of_a_mask_that_is_not_8_byte_aligned(gpu_ctx):
    T = gpu_ctx.SCAN_TILE
    keep = (np.random.default_rng(3).random(2 * T + 9) < 0.6).astype(np.uint8)
    d_keep, d_pos = _up(gpu_ctx, keep, offset=3), gpu_ctx.buffer((keep.size + 1) * 8)
    gpu_ctx.keep_positions_dev(d_keep.ptr + 3, keep.size, d_pos.ptr)
    assert np.array_equal(d_pos.download((keep.size + 1,), np.int64), up.keep_positions(keep))
    d_keep.free(), d_pos.free()


def test_keep_mask_from_removed_indices(gpu_ctx):
    rng = np.random.default_rng(4)
    for n, removed in ((1, [0]), (5, []), (5000, rng.choice(5000, 700, replace=False)), (300, [0, 1, 298, 299, 299, -1, 300])):
        removed = np.asarray(removed, np.int64)
        d_r, d_keep = _up(gpu_ctx, removed), _up(gpu_ctx, np.zeros(n, np.uint8), GUARD)
        gpu_ctx.keep_mask_dev(d_r.ptr if removed.size else None, removed.size, n, d_keep.ptr)
        got = d_keep.download((n + GUARD,), np.uint8)
        assert np.array_equal(got[:n], up.keep_mask(removed, n)) and (got[n:] == 0xA5).all()
        d_r.free(), d_keep.free()


# ------------------------------------------------------------------------------------------------ row compaction
def _compact_case(ctx, rows, keep, in_place, offset=0, first=0):
    n, rb = rows.shape
    pos = up.keep_positions(keep)
    d_keep, d_pos = _up(ctx, keep), _up(ctx, pos)
    d_rows = _up(ctx, rows, GUARD, offset)
    d_out = d_rows if in_place else _up(ctx, np.zeros_like(rows), GUARD, offset)
    ctx.compact_rows_dev(d_rows.ptr + offset, n, rb, d_keep.ptr, d_pos.ptr, d_out.ptr + offset, first=first)
    kept = int(pos[-1])
    got = d_out.download((kept, rb), np.uint8, offset=offset) if kept else np.zeros((0, rb), np.uint8)
    guard = d_out.download((GUARD,), np.uint8, offset=offset + n * rb)
    src = d_rows.download((n, rb), np.uint8, offset=offset)
    for b in {d_keep, d_pos, d_rows, d_out}:
        b.free()
    assert (guard == 0xA5).all(), "wrote past the matrix"
    assert np.array_equal(got, up.compact_rows(rows, keep, pos))
    if not in_place:
        assert np.array_equal(src, rows), "the source changed"
    removed = np.flatnonzero(keep == 0)
    head = int(removed[0]) if removed.size else n
    assert np.array_equal(got[:head], rows[:head])                   # the rows before the first removed one


@pytest.mark.parametrize("row_bytes", [1, 3, 4, 16, 24, 64, 131072])
@pytest.mark.parametrize("in_place", [False, True])
def test_compaction_at_every_move_width(gpu_ctx, row_bytes, in_place):
    n = 300 if row_bytes < 131072 else 70
    rng = np.random.default_rng(row_bytes + in_place)
    rows = rng.integers(0, 256, (n, row_bytes)).astype(np.uint8)
    for name, keep in _masks(n, 40).items():
        removed = np.flatnonzero(keep == 0)
        _compact_case(gpu_ctx, rows, keep, in_place, first=int(removed[0]) if removed.size and in_place else 0)
    _compact_case(gpu_ctx, rows, _masks(n, 40)["random bytes"], in_place, offset=4)      # both bases 4 bytes off 16-byte alignment
    _compact_case(gpu_ctx, rows[:1], np.ones(1, np.uint8), in_place)
    _compact_case(gpu_ctx, rows[:1], np.zeros(1, np.uint8), in_place)


@pytest.mark.parametrize("window", [1, 7, 64, 0])
def test_in_place_compaction_at_window_seams(gpu_ctx, window):
    from pvsim import _ffi
    rng = np.random.default_rng(50 + window)
    with gpu_ctx.option(_ffi.OPT_UPDATE_WINDOW_ROWS, window):
        assert gpu_ctx.get_option(_ffi.OPT_UPDATE_WINDOW_ROWS) == window
        for rb in (3, 16, 24):
            rows = rng.integers(0, 256, (301, rb)).astype(np.uint8)
            for name, keep in _masks(301, 64).items():
                removed = np.flatnonzero(keep == 0)
                for first in {0, int(removed[0]) if removed.size else 0}:
                    _compact_case(gpu_ctx, rows, keep, True, first=first)
    assert gpu_ctx.get_option(_ffi.OPT_UPDATE_WINDOW_ROWS) == 0
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(ValueError):
            gpu_ctx.set_option(_ffi.OPT_UPDATE_WINDOW_ROWS, bad)


def test_overlapping_out_is_refused_before_any_launch(gpu_ctx):
    rows = np.random.default_rng(6).integers(0, 256, (50, 16)).astype(np.uint8)
    keep = np.ones(50, np.uint8)
    keep[::3] = 0
    d_rows, d_keep, d_pos = _up(gpu_ctx, rows, 64), _up(gpu_ctx, keep), _up(gpu_ctx, up.keep_positions(keep))
    for shift in (16, -16 + 50 * 16, 8):
        with pytest.raises(ValueError, match="overlaps"):
            gpu_ctx.compact_rows_dev(d_rows.ptr, 50, 16, d_keep.ptr, d_pos.ptr, d_rows.ptr + shift)
    with pytest.raises(ValueError, match="overlaps"):
        gpu_ctx.compact_rows_dev(d_rows.ptr, 50, 1, d_keep.ptr, d_pos.ptr, d_keep.ptr)
    with pytest.raises(ValueError, match="overlaps"):
        gpu_ctx.copy_dev(d_rows.ptr + 8, d_rows.ptr, 100)
    gpu_ctx.sync()
    assert np.array_equal(d_rows.download((50, 16), np.uint8), rows) and np.array_equal(d_keep.download((50,), np.uint8), keep)
    d_copy = gpu_ctx.buffer(rows.nbytes)
    gpu_ctx.copy_dev(d_copy.ptr, d_rows.ptr, rows.nbytes)
    assert np.array_equal(d_copy.download(rows.shape, np.uint8), rows)
    for b in (d_rows, d_keep, d_pos, d_copy):
        b.free()


# ------------------------------------------------------------------------------------------------ inverted lists
def _stored(rng, lists, nlist, m):
    from pvsim.compact import _sort_into_lists
    n = lists.size
    codes, inv = rng.integers(0, 256, (n, m)).astype(np.uint8), rng.random(n).astype(np.float32)
    ids, off = _sort_into_lists(lists.astype(np.int64), nlist)
    return codes[ids], inv[ids], ids, off


def _list_states(rng, nlist, n):
    """list numbers of n rows: spread, all in the first / last / one middle list, and with empty lists before and after"""
    yield "spread", rng.integers(0, nlist, n)
    yield "first", np.zeros(n, np.int64)
    yield "last", np.full(n, nlist - 1)
    yield "middle", np.full(n, nlist // 2)
    if nlist >= 5:
        yield "gaps", rng.integers(2, nlist - 2, n)


def _insert_dev(ctx, nlist, m, codes, inv, ids, off, new_codes, new_inv, new_lists):
    n, b = ids.size, new_lists.size
    perm, new_off = up.sort_new_rows(new_lists, nlist)
    ins = [_up(ctx, a) for a in (codes, inv, ids, off, new_codes, new_inv, new_off, perm)]
    outs = [_up(ctx, np.zeros(s, np.uint8), GUARD) for s in ((n + b) * m, (n + b) * 4, (n + b) * 4, (nlist + 1) * 8)]
    ctx.ivf_insert_dev(m, nlist, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, off, ins[4].ptr, ins[5].ptr, ins[6].ptr, new_off,
                       ins[7].ptr, *(o.ptr for o in outs))
    got = (outs[0].download((n + b, m), np.uint8), outs[1].download((n + b,), np.float32), outs[2].download((n + b,), np.int32),
           outs[3].download((nlist + 1,), np.int64))
    for o, g in zip(outs, got):
        assert (o.download((GUARD,), np.uint8, offset=g.nbytes) == 0xA5).all()
    for x in ins + outs:
        x.free()
    want = up.ivf_insert(codes, inv, ids, off, new_codes, new_inv, new_off, perm)
    for g, w in zip(got, want):
        assert _same(g, w)


def _remove_dev(ctx, nlist, m, codes, inv, ids, off, keep):
    n = ids.size
    left = int((keep != 0).sum())
    ins = [_up(ctx, a) for a in (codes, inv, ids, off, keep, up.keep_positions(keep))]
    outs = [_up(ctx, np.zeros(s, np.uint8), GUARD) for s in (left * m, left * 4, left * 4, (nlist + 1) * 8)]
    ctx.ivf_remove_dev(m, nlist, n, *(x.ptr for x in ins), *(o.ptr for o in outs))
    got = (outs[0].download((left, m), np.uint8), outs[1].download((left,), np.float32), outs[2].download((left,), np.int32),
           outs[3].download((nlist + 1,), np.int64))
    for o, g in zip(outs, got):
        assert (o.download((GUARD,), np.uint8, offset=g.nbytes) == 0xA5).all()
    for x in ins + outs:
        x.free()
    for g, w in zip(got, up.ivf_remove(codes, inv, ids, off, keep)):
        assert _same(g, w)


@pytest.mark.parametrize("nlist", [1, 7, 300])
@pytest.mark.parametrize("m", [1, 3, 8, 64])
def test_list_insert_matches_twin(gpu_ctx, nlist, m):
    rng = np.random.default_rng(100 * nlist + m)
    for n in (0, 150):
        for _, old_lists in _list_states(rng, nlist, n):
            codes, inv, ids, off = _stored(rng, old_lists, nlist, m)
            for b in (0, 1, 40):
                for _, new_lists in _list_states(rng, nlist, b):
                    new_codes, new_inv = rng.integers(0, 256, (b, m)).astype(np.uint8), rng.random(b).astype(np.float32)
                    _insert_dev(gpu_ctx, nlist, m, codes, inv, ids, off, new_codes, new_inv, new_lists)
                    if b == 0:
                        break


@pytest.mark.parametrize("nlist", [1, 7, 300])
@pytest.mark.parametrize("m", [1, 3, 8, 64])
def test_list_remove_matches_twin(gpu_ctx, nlist, m):
    rng = np.random.default_rng(200 * nlist + m)
    n = 150
    for _, lists in _list_states(rng, nlist, n):
        codes, inv, ids, off = _stored(rng, lists, nlist, m)
        masks = _masks(n, 40)
        k = np.ones(n, np.uint8)
        k[[0, 1, n - 2, n - 1]] = 0                                  # removed ids adjacent and at both ends
        masks["ends"] = k
        k = np.ones(n, np.uint8)
        k[lists == lists[n // 2]] = 0                                # a remove that empties a list
        masks["a list emptied"] = k
        for name, keep in masks.items():
            _remove_dev(gpu_ctx, nlist, m, codes, inv, ids, off, keep)
    _remove_dev(gpu_ctx, nlist, m, *_stored(rng, np.zeros(1, np.int64), nlist, m), np.zeros(1, np.uint8))      # the index is emptied
    _remove_dev(gpu_ctx, nlist, m, *_stored(rng, np.zeros(0, np.int64), nlist, m), np.zeros(0, np.uint8))


# ------------------------------------------------------------------------------------------------ the classes against a rebuild
class _Identity:
    def encode(self, v):
        return v


def _corpus(seed, L, n=480):
    """ordinary seeded float32 rows around a few directions, and their paths"""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((9, L))
    x = (proto[rng.integers(0, 9, n)] + 0.7 * rng.standard_normal((n, L))).astype(np.float32)
    return x, [f"img/{i:04d}.jpg" for i in range(n)]


def _tables(seed, L, d, m=8, ksub=16, nlist=7):
    rng = np.random.default_rng(seed)
    w = None if d == L else np.linalg.qr(rng.standard_normal((L, d)))[0].T.astype(np.float32).copy()
    cb = (0.4 * rng.standard_normal((m, ksub, d // m))).astype(np.float32)
    cent = rng.standard_normal((nlist, d)).astype(np.float32)
    cent[3] = 50.0                                                  # no row comes near it: list 3 stays empty
    return w, cb, cent


def _build(ctx, kind, x, paths, w, cb, cent, project):
    """the public constructor fed with arrays computed at once over the rows, through the public pieces and the given tables"""
    from pvsim import CompactIndex, IVFCompactIndex, ProductQuantizer
    from pvsim.compact import _sort_into_lists
    pq = ProductQuantizer.from_codebooks(cb, ctx)
    n, d = len(paths), pq.d
    y = project(x) if n else np.zeros((0, d), np.float32)
    d_y, d_inv = _up(ctx, y), ctx.buffer(max(n * 4, 16))
    if n:
        ctx.row_inv_norms_dev(d_y.ptr, n, d, d_inv.ptr)
    inv = d_inv.download((n,), np.float32)
    if kind == "flat":
        d_y.free(), d_inv.free()
        return CompactIndex(paths, pq.encode(y), inv, pq, w, y, ctx)
    nlist = cent.shape[0]
    d_cent, d_lists, d_res = _up(ctx, cent), ctx.buffer(max(n * 4, 16)), ctx.buffer(max(n * d * 4, 16))
    if n:
        ctx.ivf_assign_dev(d_y.ptr, n, d, d_cent.ptr, nlist, d_lists.ptr, d_res.ptr)
    lists, res = d_lists.download((n,), np.int32), d_res.download((n, d), np.float32)
    for b in (d_y, d_inv, d_cent, d_lists, d_res):
        b.free()
    ids, off = _sort_into_lists(lists, nlist)
    return IVFCompactIndex(paths, pq.encode(res)[ids], inv[ids], pq, cent, off, ids, w, y, ctx)


def _assert_same_index(index, ref, queries, kind):
    from pvsim import eval as ev
    assert index.paths == ref.paths and len(index) == len(ref) and index.keys() == ref.keys()
    for got, want in zip(index._download(), ref._download()):
        assert _same(got, want)
    assert index.nbytes_breakdown == ref.nbytes_breakdown
    n = len(index)
    if kind == "ivf":
        assert _same(index._list_off, ref._list_off) and _same(index._ids, ref._ids) and _same(index.list_sizes, ref.list_sizes)
        assert _same(index._device()["list_off"].download((index.nlist + 1,), np.int64), ref._list_off)
    if n == 0:
        return
    k, R = min(10, n), min(30, n)
    for extra in ([dict(nprobe=p) for p in (1, 3, index.nlist)] if kind == "ivf" else [{}]):
        for rr in (0, R):
            gi, gv = index.rank(queries, k, rerank=rr, **extra)
            wi, wv = ref.rank(queries, k, rerank=rr, **extra)
            assert _same(gi, wi) and _same(gv, wv), (kind, extra, rr)
    extra = dict(nprobe=3) if kind == "ivf" else {}
    for q in queries[:2]:
        got = ev.retrieve_top_k_similar(q, index, _Identity(), k=k, rerank=R, **extra)
        want = ev.retrieve_top_k_similar(q, ref, _Identity(), k=k, rerank=R, **extra)
        assert [p for p, _ in got] == [p for p, _ in want] and _same(np.array([s for _, s in got]), np.array([s for _, s in want]))


@pytest.mark.parametrize("kind", ["flat", "ivf"])
@pytest.mark.parametrize("L,d", [(64, 64), (256, 64)])
def test_compact_indexes_after_updates_equal_a_rebuild(gpu_ctx, kind, L, d, tmp_path):
    from pvsim import CompactIndex, IVFCompactIndex
    x, paths = _corpus(7000 + L, L)
    w, cb, cent = _tables(7100 + L, L, d)
    bare = _build(gpu_ctx, "flat", x[:0], [], w, cb, cent, None)     # an empty index with the same projection: its `project` is the public piece
    project = bare.project
    index = _build(gpu_ctx, kind, x[:300], paths[:300], w, cb, cent, project)
    alive = list(range(300))
    rng = np.random.default_rng(7200)
    gone = sorted({0, 419} | set(rng.choice(420, 140, replace=False).tolist()))
    queries = np.ascontiguousarray(np.concatenate([x[[5, 77]], x[[gone[3]]], x[[430]], rng.standard_normal((2, L)).astype(np.float32)]))

    def check():
        ref = _build(gpu_ctx, kind, x[alive], [paths[i] for i in alive], w, cb, cent, project)
        _assert_same_index(index, ref, queries, kind)
        ref.close()

    check()                                                         # ranks with rerank= before any update: the caches exist from here on
    steps = [("add", range(300, 320)), ("add", range(320, 420)), ("remove", gone), ("add", range(420, 480))]
    for op, rows in steps:
        rows = list(rows)
        if op == "add":
            before = index._device()["codes"].nbytes
            index.add({paths[i]: x[i] for i in rows})
            alive += rows
            if kind == "flat" and rows[0] == 300:
                assert index._device()["codes"].nbytes > before          # this add outgrew the buffers
        else:
            index.remove([paths[i] for i in reversed(rows)])           # any order of naming
            alive = [i for i in alive if i not in set(rows)]
        check()
    index.add({})
    index.remove([])
    with pytest.raises(ValueError, match="already indexed"):
        index.add({paths[alive[3]]: x[0]})
    with pytest.raises(KeyError):
        index.remove([paths[gone[0]]])
    check()
    # persistence: arrays sized n, not capacity
    fn = str(tmp_path / f"{kind}.npz")
    index.save(fn)
    back = (CompactIndex if kind == "flat" else IVFCompactIndex).load(fn, gpu_ctx)
    _assert_same_index(back, index, queries, kind)
    back.close()
    # a resident DeviceIndex as the source, then everything leaves and something returns
    from pvsim.index import DeviceIndex
    tail = DeviceIndex({f"more/{i}": x[i] for i in range(10)}, gpu_ctx)
    index.add(tail)
    tail.close()
    ref = _build(gpu_ctx, kind, np.concatenate([x[alive], x[:10]]), [paths[i] for i in alive] + [f"more/{i}" for i in range(10)], w, cb,
                 cent, project)
    _assert_same_index(index, ref, queries, kind)
    ref.close()
    del index["more/3"]
    index.remove(index.paths)
    assert len(index) == 0 and index.paths == []
    ref = _build(gpu_ctx, kind, x[:0], [], w, cb, cent, project)
    _assert_same_index(index, ref, queries, kind)
    ref.close()
    index.add({paths[i]: x[i] for i in range(40)})
    alive = list(range(40))
    check()
    index.close(), bare.close()


def test_a_fitted_ivf_index_takes_updates(gpu_ctx):
    from pvsim import IVFCompactIndex
    x, paths = _corpus(7300, 64, 400)
    index = IVFCompactIndex.fit({p: v for p, v in zip(paths[:300], x[:300])}, 5, m=8, ksub=16, keep_projected=True, random_state=3,
                                max_iter=4, ctx=gpu_ctx)
    index.rank(x[:2], 5, 2, rerank=20)
    index.add({p: v for p, v in zip(paths[300:], x[300:])})
    index.remove(paths[100:250] + paths[:1])
    alive = list(range(1, 100)) + list(range(250, 400))
    ref = _build(gpu_ctx, "ivf", x[alive], [paths[i] for i in alive], None, index.quantizer.codebooks, index.centroids, lambda r: r.copy())
    _assert_same_index(index, ref, np.ascontiguousarray(x[[3, 120, 399]]), "ivf")
    ref.close(), index.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_index_after_updates_equals_a_rebuild(gpu_ctx, dtype):
    from pvsim import QueryExpansion
    from pvsim.index import DeviceIndex
    from pvsim import eval as ev
    x, paths = _corpus(7400, 64)
    x = x.astype(dtype)
    rng = np.random.default_rng(7401)
    gone = sorted({0, 419} | set(rng.choice(420, 140, replace=False).tolist()))
    queries = np.ascontiguousarray(np.concatenate([x[[5, 77]], x[[gone[3]]], x[[430]], rng.standard_normal((2, 64)).astype(dtype)]))
    index = DeviceIndex({paths[i]: x[i] for i in range(300)}, gpu_ctx)
    alive = list(range(300))
    old = index.augmented(r=3)

    def check():
        ref = DeviceIndex({paths[i]: x[i] for i in alive}, gpu_ctx)
        assert len(index) == len(ref) and list(index) == list(ref) and list(index.keys()) == [paths[i] for i in alive]
        assert _same(index.matrix, ref.matrix) and _same(index.inv_norms, ref.inv_norms)
        for i in (alive[0], alive[len(alive) // 2], alive[-1]):
            assert _same(index[paths[i]], x[i]) and paths[i] in index
        k = min(10, len(alive))
        for got, want in zip(index.rank(queries, k), ref.rank(queries, k)):
            assert _same(got, want)
        for got, want in zip(index.rank_expanded(queries, k, QueryExpansion(n=5)), ref.rank_expanded(queries, k, QueryExpansion(n=5))):
            assert _same(got, want)
        got = ev.retrieve_top_k_similar(queries[0], index, _Identity(), k=k)
        want = ev.retrieve_top_k_similar(queries[0], ref, _Identity(), k=k)
        assert [p for p, _ in got] == [p for p, _ in want] and _same(np.array([s for _, s in got]), np.array([s for _, s in want]))
        ref.close()

    check()
    for op, rows in (("add", range(300, 320)), ("add", range(320, 420)), ("remove", gone), ("add", range(420, 480))):
        rows = list(rows)
        if op == "add":
            cap = index.capacity
            index.add({paths[i]: x[i] for i in rows})
            alive += rows
            assert (index.capacity > cap) == (rows[0] == 300) or rows[0] == 420      # the first add outgrows the buffers, the second fits
        else:
            index.remove([paths[i] for i in reversed(rows)])
            alive = [i for i in alive if i not in set(rows)]
            assert paths[rows[0]] not in index
        check()
    del index[paths[alive[7]]]
    alive.pop(7)
    index.reserve(2000)
    assert index.capacity == 2000
    index.add({})
    index.remove([])
    check()
    assert len(old) == 300 and list(old) == paths[:300]               # an index returned earlier by augmented() is a separate index
    # several updates before anyone asks for host rows: the mirror's notes are applied in order
    index.remove([paths[i] for i in alive[10:60]])
    index.add({f"late/{i}": x[i] for i in range(5)})
    index.remove([paths[alive[0]], "late/2", paths[alive[-1]]])
    index.add({f"later/{i}": x[100 + i] for i in range(3)})
    assert len(index._pending) == 4
    rows = [x[i] for i in alive[1:10] + alive[60:-1]] + [x[i] for i in (0, 1, 3, 4)] + [x[100 + i] for i in range(3)]
    names = [paths[i] for i in alive[1:10] + alive[60:-1]] + [f"late/{i}" for i in (0, 1, 3, 4)] + [f"later/{i}" for i in range(3)]
    ref = DeviceIndex(dict(zip(names, rows)), gpu_ctx)
    for got, want in zip(index.rank(queries, 10), ref.rank(queries, 10)):       # the device did not wait for the mirror
        assert _same(got, want)
    assert len(index._pending) == 4 and _same(index.inv_norms, ref.inv_norms)
    assert list(index) == names and _same(index.matrix, ref.matrix) and index._pending == [] and _same(index["late/3"], x[3])
    ref.close()
    index.remove(list(index))
    assert len(index) == 0 and index.matrix.shape == (0, 64) and index.inv_norms.shape == (0,)
    index.add({paths[i]: x[i] for i in range(30)})
    alive = list(range(30))
    check()
    index.close(), old.close()


def _small_updated_index(ctx, dtype):
    """a DeviceIndex of 40 x 16 rows after a remove of 3 scattered paths and an add of 5 -> (index, dict of the survivors in order,
    rows); its host mirror is behind by those two updates"""
    from pvsim.index import DeviceIndex
    x, paths = _corpus(7500, 16, n=45)
    x = x.astype(dtype)
    index = DeviceIndex({paths[i]: x[i] for i in range(40)}, ctx)
    index.remove([paths[i] for i in (31, 2, 17)])
    index.add({paths[i]: x[i] for i in range(40, 45)})
    alive = [i for i in range(45) if i not in (2, 17, 31)]
    assert len(index._pending) == 2 and list(index) == [paths[i] for i in alive]
    return index, {paths[i]: x[i] for i in alive}, x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_leaves_the_host_mirror_of_an_updated_index_alone(gpu_ctx, dtype):
    """the retrieval functions rank a resident index on the device and read its paths: the rows an update left behind in the host
    mirror are not compacted for them, and the results are those of the dict of the survivors"""
    from pvsim import eval as ev
    index, survivors, x = _small_updated_index(gpu_ctx, dtype)
    labels = {p: i % 4 for i, p in enumerate(survivors)}
    queries, q_labels = [x[5], x[2], x[41], x[30]], [1, 0, 3, 2]
    for target in (index, survivors):
        got = [ev.retrieve_top_k_similar(queries[0], target, _Identity(), k=7),
               ev.retrieve_top_k_similar(queries[1], target, _Identity(), k=100),
               ev.top_k_map(queries, q_labels, target, labels, _Identity(), k=9),
               ev.top_k_map(queries, q_labels, target, labels, _Identity()),
               ev.top_k_accuracy(queries, q_labels, target, labels, _Identity(), k=3)]
        if target is index:
            assert len(index._pending) == 2                         # nobody asked for host rows
            resident = got
    assert len(resident[1]) == 42
    for a, b in zip(resident[:2], got[:2]):
        assert [p for p, _ in a] == [p for p, _ in b] and _same(np.array([s for _, s in a]), np.array([s for _, s in b]))
    assert resident[2:] == got[2:]
    index.close()


def test_expand_verified_after_an_update(gpu_ctx):
    """the members' positions come from the index's own path ledger: the list equals the one the dict of the survivors gives"""
    from pvsim import QueryExpansion
    from pvsim import eval as ev
    index, survivors, x = _small_updated_index(gpu_ctx, np.float32)
    names = list(survivors)
    ranked = [(names[1], 0.9, 12), (names[20], 0.8, 2), (names[-1], 0.7, 9), (names[5], 0.6, 0)]     # two verified: one old, one added
    got = ev.expand_verified(x[5], ranked, index, _Identity(), k=6, qe=QueryExpansion(n=3))
    want = ev.expand_verified(x[5], ranked, survivors, _Identity(), k=6, qe=QueryExpansion(n=3))
    assert len(got) == 6 and [p for p, _ in got] == [p for p, _ in want]
    assert _same(np.array([s for _, s in got]), np.array([s for _, s in want]))
    assert len(index._pending) == 2
    index.close()
