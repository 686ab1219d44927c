"""GPU tests of subset search (csrc/subset.hip, pvsim/subset.py) against the NumPy twin (tests/subset_numpy.py).
A subset ranking is the full ranking with the rows outside S deleted, and its scores are the full ranking's, so every comparison is
np.array_equal on bytes: exact lattice rows and integer code rows against the twin, seeded Gaussian rows against the index's own
unrestricted `rank` filtered on the host.  Every case runs on both paths and auto, with the plan's geometry and with tiles of 48 and 64
(at 48 a panel starts off a mask word, and there are several row blocks, column panels and chunks)."""
import numpy as np
import pytest

import range_numpy as rn
import sq8_numpy as sq
import subset_numpy as tw
from pvsim import Subset                       # the feature itself: without it nothing in this file can run

pytestmark = pytest.mark.gpu

OPT_SQ8_PATH = 7
SUBSET_PATHS = (0, 1, 2)                       # auto, mask, listed
TILES = (0, 48, 64)
NQS = (1, 4, 5, 129)
NQ_MAX = 129


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sets(N, best):
    """the allowed sets of the issue, duplicates dropped (a small N makes some of them equal): name -> sorted ids"""
    sets = {"first": [0], "last": [N - 1], "even": list(range(0, N, 2)), "dups": [1, 2], "no_best": [i for i in range(N) if i != best],
            "all": list(range(N)), "empty_tile": [i for i in range(N) if not 48 <= i < 128]}      # [48, 96) and [64, 128) hold no id
    out, seen = {}, set()
    for name, ids in sets.items():
        if tuple(ids) not in seen and ids:
            seen.add(tuple(ids))
            out[name] = np.array(ids, np.int64)
    return out


def _ks(ns):
    return sorted({k for k in (1, 2, 16, 17, ns) if k <= min(ns, 1024)})


class _Lists:
    """device output lists of NQ_MAX queries, reused by every call of a test"""

    def __init__(self, ctx, kmax):
        self.idx, self.val = ctx.buffer(NQ_MAX * kmax * 8), ctx.buffer(NQ_MAX * kmax * 4)

    def get(self, nq, k):
        return self.idx.download((nq, k), np.int64), self.val.download((nq, k), np.float32)

    def free(self):
        self.idx.free(), self.val.free()


def _check(got, want, nq, k, what):
    assert np.array_equal(got[0], want[0][:nq, :k]), what + (np.argwhere(got[0] != want[0][:nq, :k])[:4].tolist(),)
    assert np.array_equal(_bits(got[1]), _bits(want[1][:nq, :k])), what


# ------------------------------------------------------------------------------------------------ float32 index, exact rows
def _lattice_case(ctx, N, L):
    from pvsim.index import DeviceIndex
    x = rn.lattice(N, L, 100 + N + L)
    q = rn.lattice(NQ_MAX, L, 200 + N + L)
    q[0] = x[0]                                 # rows 0, 1, 2 tie at 1 for query 0, row 3 is its worst, row 4 scores 0; query 4 is zero
    index = DeviceIndex({f"p{i:04d}": x[i] for i in range(N)}, ctx)
    return index, x, q, rn.lattice_scores(q, x)


@pytest.mark.parametrize("N,L", [(N, L) for N in (5, 33, 127, 128, 129, 1000) for L in (16, 64, 1000)] + [(129, 18)])
def test_float32_lists_equal_the_twin_on_every_path_and_seam(gpu_ctx, N, L):
    """lattice rows, whose scores are exact: every set, nq, k, path and tile; S = all rows also equals index.rank(q, k).
    L = 18 takes the generic (L % 4 != 0) scorer, once."""
    ctx = gpu_ctx
    index, x, q, scores = _lattice_case(ctx, N, L)
    assert np.array_equal(index.inv_norms, rn.lattice_inv(x))
    best = int(tw.restricted_topk(scores[:1], range(N), 1)[0][0, 0])
    assert best == 0 and scores[0, 1] == scores[0, 2] == 1 and scores[0, 3] == -1
    d_q, d_invq, out = ctx.buffer(q.nbytes).upload(q), ctx.buffer(NQ_MAX * 4), _Lists(ctx, min(N, 1024))
    index._row_inv_norms(d_q.ptr, NQ_MAX, d_invq.ptr)
    plain = {(nq, k): index.rank(q[:nq], k) for nq in NQS for k in _ks(N)}
    for name, ids in _sets(N, best).items():
        want = tw.restricted_topk(scores, ids, min(ids.size, 1024))
        handle = ctx.subset_create(ids, N)
        for nq in NQS:
            for k in _ks(ids.size):
                for path in SUBSET_PATHS:
                    for tile in TILES:
                        st = ctx.cosine_topk_subset_dev(d_q.ptr, nq, index._db.ptr, N, L, d_invq.ptr, index._inv.ptr, handle, k, out.idx.ptr,
                                                        out.val.ptr, path=path, tile=tile)
                        got = out.get(nq, k)
                        _check(got, want, nq, k, (N, L, name, nq, k, path, tile))
                        assert st["path"] in ("mask", "listed") and (path == 0 or st["path"] == ("mask", "listed")[path - 1])
                        assert set(np.unique(got[0]).tolist()) <= set(ids.tolist())
                        if name == "all":
                            assert np.array_equal(got[0], plain[nq, k][0]) and np.array_equal(_bits(got[1]), _bits(plain[nq, k][1]))
        handle.close()
    if N >= 5:                                  # the tie among the duplicates is decided inside S: 1 before 2, without row 0
        assert tw.restricted_topk(scores[:1], [1, 2], 2)[0][0].tolist() == [1, 2]
    for b in (d_q, d_invq):
        b.free()
    out.free()
    index.close()


@pytest.mark.parametrize("L", [64, 1000])
def test_float32_lists_equal_the_filtered_full_ranking_on_gaussian_rows(gpu_ctx, L):
    """no twin predicts these bits: the lists must be index.rank(q, N) -- the unrestricted code -- filtered to S and cut"""
    from pvsim.index import DeviceIndex
    from pvsim.subset import rank_subset
    rng = np.random.default_rng(5 + L)
    N = 1000
    x = rng.standard_normal((N, L)).astype(np.float32)
    x[7] = x[3]                                                          # one exact tie
    qs = rng.standard_normal((513, L)).astype(np.float32)
    qs[0] = x[3]
    index = DeviceIndex({f"p{i:04d}": x[i] for i in range(N)}, gpu_ctx)
    for nq in (1, 5, 129, 513):                                          # rank takes its one-pass, plain and prefiltered forms
        full_i, full_v = index.rank(qs[:nq], N)
        best = int(full_i[0, 0])
        for name, ids in _sets(N, best).items():
            keep = np.isin(full_i, ids)
            want_i = full_i[keep].reshape(nq, ids.size)
            want_v = full_v[keep].reshape(nq, ids.size)
            with index.subset(ids) as sub:
                for k in sorted({1, min(17, ids.size), ids.size}):
                    for path, tile in (("mask", 0), ("listed", 0), ("mask", 48), ("listed", 48), ("auto", 0)):
                        if nq == 513 and tile:
                            continue                                     # 11 row blocks x 21 panels add nothing to the seams above
                        got = rank_subset(index, qs[:nq], k, sub, path, tile)
                        _check(got, (want_i, want_v), nq, k, (L, nq, name, k, path, tile))
    index.close()


# ------------------------------------------------------------------------------------------------ int8 index
def _code_rows(nq, N, L):
    """asymmetric integer code rows of the kind test_gpu_sq8.py ranks: queries and rows follow different patterns; planted duplicates
    (rows N - 1 = 0 and 2 = 1: exact ties, decided by the index) and, where 127^2 L exceeds 2^24, rows 5 and 9 whose sums with query 0
    differ by one and collapse to one float"""
    ld = sq.ld_of(L)
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
    iq, idb = sq.factors(qc), sq.factors(dc)
    if collapse:
        idb[9] = idb[5]
        a = sq.acc(qc[:1], dc[[5, 9]])[0]
        assert a[0] == a[1] + 1 and a[1] > 2 ** 24 and np.float32(np.int32(a[0])) == np.float32(np.int32(a[1]))
    return qc, iq, dc, idb


@pytest.mark.parametrize("sq8_path", [0, 1, 2])
@pytest.mark.parametrize("N,L", [(5, 1), (5, 64), (129, 1), (129, 64), (129, 65), (129, 1000), (129, 2048), (1000, 64), (1000, 65), (1000, 1000)])
def test_int8_lists_equal_the_twin_on_every_path_and_seam(gpu_ctx, N, L, sq8_path):
    """integer code rows against sq8_numpy.scores + restricted_topk: the sets, paths and tiles of the float32 test, under every
    PVS_OPT_SQ8_PATH (nq = 4 and 5 stand on either side of its own cut).  L = 2048 brings the pair of sums above 2^24 that collapse
    to one float: 127^2 L stays below 2^24 at the other lengths."""
    ctx = gpu_ctx
    qc, iq, dc, idb = _code_rows(NQ_MAX, N, L)
    scores = sq.scores(qc, iq, dc, idb)
    best = int(tw.restricted_topk(scores[:1], range(N), 1)[0][0, 0])
    bufs = [ctx.buffer(max(a.nbytes, 16)).upload(a) for a in (qc, iq, dc, idb)]
    out = _Lists(ctx, min(N, 1024))
    with ctx.option(OPT_SQ8_PATH, sq8_path):
        for name, ids in _sets(N, best).items():
            want = tw.restricted_topk(scores, ids, min(ids.size, 1024))
            handle = ctx.subset_create(ids, N)
            for nq in NQS:
                for k in _ks(ids.size):
                    for path in SUBSET_PATHS:
                        for tile in TILES:
                            ctx.sq8_topk_subset_dev(bufs[0].ptr, bufs[1].ptr, nq, bufs[2].ptr, bufs[3].ptr, N, L, handle, k, out.idx.ptr,
                                                    out.val.ptr, path=path, tile=tile)
                            _check(out.get(nq, k), want, nq, k, (N, L, sq8_path, name, nq, k, path, tile))
                if name == "all":                # S = all rows: the unrestricted entry's lists
                    for k in _ks(N):
                        ctx.sq8_topk_dev(bufs[0].ptr, bufs[1].ptr, nq, bufs[2].ptr, bufs[3].ptr, N, L, k, 0, False, out.idx.ptr, out.val.ptr)
                        _check(out.get(nq, k), want, nq, k, (N, L, sq8_path, "plain", nq, k))
            handle.close()
    if L >= 2000:                                # the collapsed pair ties: 5 before 9, inside a set that holds both and not the rows between
        i, v = tw.restricted_topk(scores[:1], [5, 9], 2)
        assert i[0].tolist() == [5, 9] and _bits(v)[0, 0] == _bits(v)[0, 1]
    for b in bufs:
        b.free()
    out.free()


# ------------------------------------------------------------------------------------------------ the C entries
def _call_f32(ctx, c, handle, nq, N, k, path=0, tile=0):
    return ctx.cosine_topk_subset_dev(c["q"].ptr, nq, c["x"].ptr, N, c["L"], c["iq"].ptr, c["ix"].ptr, handle, k, c["idx"].ptr, c["val"].ptr,
                                      path=path, tile=tile)


def _call_i8(ctx, c, handle, nq, N, k, path=0, tile=0):
    return ctx.sq8_topk_subset_dev(c["qc"].ptr, c["iqc"].ptr, nq, c["dc"].ptr, c["idc"].ptr, N, c["L"], handle, k, c["idx"].ptr, c["val"].ptr,
                                   path=path, tile=tile)


@pytest.fixture(scope="module")
def entry_case(gpu_ctx):
    """200 lattice rows and 130 queries of 64 dims, and the int8 codes of both, resident for the entry-point tests"""
    ctx, N, nq, L = gpu_ctx, 200, 130, 64
    x, q = rn.lattice(N, L, 1), rn.lattice(nq, L, 2)
    qc, iqc = sq.encode(q)
    dc, idc = sq.encode(x)
    c = {"N": N, "nq": nq, "L": L, "x_host": x, "q_host": q, "codes": (qc, iqc, dc, idc)}
    for name, a in (("q", q), ("x", x), ("iq", rn.lattice_inv(q)), ("ix", rn.lattice_inv(x)), ("qc", qc), ("iqc", iqc), ("dc", dc), ("idc", idc)):
        c[name] = ctx.buffer(a.nbytes).upload(a)
    c["idx"], c["val"] = ctx.buffer(nq * N * 8), ctx.buffer(nq * N * 4)
    yield c
    for v in c.values():
        if hasattr(v, "free"):
            v.free()


def test_subset_create_refuses_bad_ids(gpu_ctx):
    for ids, what in (([3, 1, 2], "unsorted"), ([1, 1], "a repeated id"), ([0, 10], "an id equal to N"), ([-1, 2], "a negative id"),
                      ([], "no id"), (list(range(10)) + [9], "more ids than rows")):
        with pytest.raises(ValueError, match="pvs_subset_create"):
            gpu_ctx.subset_create(np.array(ids, np.int64), 10)
    with pytest.raises(ValueError, match="pvs_subset_create"):
        gpu_ctx.subset_create(np.array([0], np.int64), 0)
    h = gpu_ctx.subset_create(np.array([0, 9], np.int64), 10)
    assert (h.n, h.size) == (10, 2)
    h.close()
    h.close()                                   # closing twice is harmless


@pytest.mark.parametrize("call", [_call_f32, _call_i8])
def test_entries_refuse_invalid_arguments_before_any_launch(gpu_ctx, entry_case, call):
    c, N = entry_case, entry_case["N"]
    h = gpu_ctx.subset_create(np.arange(0, N, 2, dtype=np.int64), N)                 # ns = 100
    other = gpu_ctx.subset_create(np.arange(0, N, 2, dtype=np.int64), N + 1)         # a handle made for another N
    before = c["idx"].download((4,), np.int64)
    for kw, what in ((dict(k=0), "k"), (dict(k=101), "k"), (dict(k=-3), "k"), (dict(path=3), "path"), (dict(path=-1), "path"),
                     (dict(tile=-1), "tile"), (dict(tile=32769), "tile")):
        with pytest.raises(ValueError, match=what):
            call(gpu_ctx, c, h, 3, N, **{"k": 5, **kw})
    with pytest.raises(ValueError, match="made for"):
        call(gpu_ctx, c, other, 3, N, 5)
    with pytest.raises(ValueError, match="made for"):
        call(gpu_ctx, c, h, 3, N - 1, 5)
    assert np.array_equal(c["idx"].download((4,), np.int64), before)                 # nothing was written
    assert call(gpu_ctx, c, h, 0, N, 5)["scored"] == 0                               # nq == 0 is a no-op
    h.close(), other.close()
    deep = gpu_ctx.subset_create(np.arange(1100, dtype=np.int64), 1100)              # k <= ns, but deeper than one page
    with pytest.raises(ValueError, match="1024"):
        call(gpu_ctx, c, deep, 1, 1100, 1025)
    deep.close()


@pytest.mark.parametrize("call", [_call_f32, _call_i8])
def test_stats_report_skipped_panels_and_gathered_rows(gpu_ctx, entry_case, call):
    c, N, nq = entry_case, entry_case["N"], entry_case["nq"]
    ids = np.array([i for i in range(N) if not 48 <= i < 128], np.int64)
    h = gpu_ctx.subset_create(ids, N)
    names = ("path", "scored", "panels_skipped", "rows_gathered")
    for tile in (48, 64):
        st = call(gpu_ctx, c, h, nq, N, 7, path=1, tile=tile)
        want = tw.mask_stats(ids, nq, N, tile, tile)
        assert [st[n] for n in names] == ["mask"] + want[1:] and st["panels_skipped"] == 3, (tile, st)
        st = call(gpu_ctx, c, h, nq, N, 7, path=2, tile=tile)
        assert [st[n] for n in names] == ["listed"] + tw.listed_stats(ids.size, tile)[1:] and st["rows_gathered"] == ids.size, (tile, st)
    st = call(gpu_ctx, c, h, nq, N, 7, path=1)
    assert [st[n] for n in names] == ["mask", 1, 0, 0]                               # one panel in the plan's geometry: nothing to skip
    st = call(gpu_ctx, c, h, nq, N, 7, path=2)
    assert [st[n] for n in names] == ["listed", 1, 0, ids.size]
    h.close()


# ------------------------------------------------------------------------------------------------ Python
class _Enc:
    context = None

    def encode(self, image):
        return np.asarray(image, np.float32).reshape(1, -1)


@pytest.fixture(scope="module")
def indexes(gpu_ctx):
    """60 lattice rows of 64 dims as a dict, a float32 DeviceIndex and an Int8Index, with both twins' score matrices for 6 queries"""
    from pvsim import Int8Index
    from pvsim.index import DeviceIndex
    x, q = rn.lattice(60, 64, 11), rn.lattice(6, 64, 12)
    q[0] = x[0]
    enc = {f"img_{i:02d}.jpg": x[i] for i in range(60)}
    dense, int8 = DeviceIndex(enc, gpu_ctx), Int8Index(enc, gpu_ctx)
    qc, iqc = sq.encode(q)
    dc, idc = sq.encode(x)
    yield {"enc": enc, "paths": list(enc), "x": x, "q": q, "dense": dense, "int8": int8, "s_dense": rn.lattice_scores(q, x),
           "s_int8": sq.scores(qc, iqc, dc, idc)}
    dense.close(), int8.close()


@pytest.mark.parametrize("kind", ["dense", "int8"])
def test_three_forms_of_allowed_give_the_same_bytes(indexes, kind):
    index, q, paths = indexes[kind], indexes["q"], indexes["paths"]
    ids = [3, 0, 41, 2, 17, 59, 1]
    want = tw.restricted_topk(indexes["s_" + kind], ids, 5)
    mask = np.isin(np.arange(60), ids)
    sub = index.subset(ids)
    assert isinstance(sub, Subset) and len(sub) == 7 and sub.ids.tolist() == sorted(ids) and sub.ids.dtype == np.int64
    for allowed in (np.array(ids), ids, mask, [paths[i] for i in ids], sub, sub):                    # the Subset is used twice
        for path in ("auto", "mask", "listed"):
            got = index.rank(q, 5, allowed=allowed, subset_path=path)
            _check(got, want, 6, 5, (kind, path))
            assert got[0].dtype == np.int64 and got[1].dtype == np.float32
            assert index.last_subset_stats["path"] == ("listed" if path == "auto" else path)          # 4 * 7 <= 60
    _check(index.rank(q, 7, allowed=sub), tw.restricted_topk(indexes["s_" + kind], ids, 7), 6, 7, (kind, "k = |S|"))
    full = index.rank(q, 60, allowed=np.ones(60, bool))
    plain = index.rank(q, 60)
    assert np.array_equal(full[0], plain[0]) and np.array_equal(_bits(full[1]), _bits(plain[1]))
    assert index.last_subset_stats["path"] == "mask"
    e = index.rank(np.zeros((0, 64), np.float32), 3, allowed=sub)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)
    for bad, exc in ((dict(k=8), ValueError), (dict(k=0), ValueError), (dict(k=2.5), ValueError), (dict(subset_path="fast"), ValueError)):
        with pytest.raises(exc):
            index.rank(q, **{"k": 3, "allowed": sub, **bad})
    with pytest.raises(ValueError, match="twice"):
        index.rank(q, 1, allowed=[4, 4])
    with pytest.raises(IndexError):
        index.rank(q, 1, allowed=[60])
    with pytest.raises(KeyError):
        index.rank(q, 1, allowed=["nope.jpg"])
    with pytest.raises(ValueError, match="empty"):
        index.rank(q, 1, allowed=np.zeros(60, bool))
    with pytest.raises(ValueError):
        index.rank(q[:, :32], 1, allowed=sub)
    with pytest.raises(TypeError, match="float32"):
        index.rank(q.astype(np.float64), 1, allowed=sub)
    sub.close()
    with pytest.raises(ValueError, match="closed"):
        index.rank(q, 1, allowed=sub)


def test_float64_index_and_foreign_subsets_are_refused(gpu_ctx, indexes):
    from pvsim.index import DeviceIndex
    f64 = DeviceIndex({p: v.astype(np.float64) for p, v in indexes["enc"].items()}, gpu_ctx)
    with pytest.raises(TypeError, match="float32"):
        f64.subset([0, 1])
    with pytest.raises(TypeError, match="float32"):
        f64.rank(indexes["q"], 1, allowed=[0, 1])
    f64.close()
    sub = indexes["dense"].subset([0, 1])
    with pytest.raises(ValueError, match="another index"):
        indexes["int8"].rank(indexes["q"], 1, allowed=sub)
    sub.close()


@pytest.mark.parametrize("kind", ["dense", "int8"])
def test_a_subset_is_a_snapshot(gpu_ctx, indexes, kind):
    from pvsim import Int8Index
    from pvsim.index import DeviceIndex
    enc, q = dict(list(indexes["enc"].items())[:20]), indexes["q"]
    index = (DeviceIndex if kind == "dense" else Int8Index)(enc, gpu_ctx)
    sub = index.subset([1, 5, 7])
    first = index.rank(q, 2, allowed=sub)
    index.reserve(64)                                                    # the rows are the same rows: the ids still name them
    again = index.rank(q, 2, allowed=sub)
    assert np.array_equal(first[0], again[0]) and np.array_equal(_bits(first[1]), _bits(again[1]))
    index.add({"new.jpg": indexes["x"][30]})
    with pytest.raises(ValueError, match="has changed"):
        index.rank(q, 2, allowed=sub)
    sub2 = index.subset([1, 5, 20])
    assert index.rank(q, 3, allowed=sub2)[0].shape == (6, 3)
    index.remove(["new.jpg"])
    with pytest.raises(ValueError, match="has changed"):
        index.rank(q, 2, allowed=sub2)
    sub3 = index.subset([0, 2])
    del index["img_00.jpg"]
    with pytest.raises(ValueError, match="has changed"):
        index.rank(q, 1, allowed=sub3)
    for s in (sub, sub2, sub3):
        s.close()
    got = index.rank(q, 2, allowed=["img_01.jpg", "img_05.jpg", "img_07.jpg"])         # the rows moved down by one; the paths still find them
    assert np.array_equal(got[0], first[0] - 1) and np.array_equal(_bits(got[1]), _bits(first[1]))
    index.close()


def test_eval_functions_rank_within_the_set(gpu_ctx, indexes):
    from pvsim import eval as ev
    paths, q = indexes["paths"], indexes["q"]
    ids = [0, 1, 2, 3, 9, 10, 30, 31, 58]
    allowed_forms = (ids, [paths[i] for i in ids], np.isin(np.arange(60), ids))
    labels = {p: i % 3 for i, p in enumerate(paths)}
    qlabels = [0, 1, 2, 0, 1, 2]
    for kind, dataset in (("dense", indexes["enc"]), ("dense", indexes["dense"]), ("int8", indexes["int8"])):
        want_i, want_v = tw.restricted_topk(indexes["s_" + kind], ids, len(ids))
        for allowed in allowed_forms + ((dataset.subset(ids),) if not isinstance(dataset, dict) else ()):
            for k in (1, 4, 9, 50):                                      # 50 is clamped to |S| = 9
                kk = min(k, len(ids))
                got = ev.retrieve_top_k_similar(q[0], dataset, _Enc(), k=k, allowed=allowed)
                assert [p for p, _ in got] == [paths[i] for i in want_i[0, :kk]], (kind, k)
                assert np.array_equal(_bits([s for _, s in got]), _bits(want_v[0, :kk])), (kind, k)
                aps, hits = [], 0
                for row, lab in zip(want_i[:, :kk], qlabels):
                    rel = [j + 1 for j, i in enumerate(row) if labels[paths[i]] == lab]
                    aps.append(sum((n + 1) / r for n, r in enumerate(rel)) / len(rel) if rel else 0.0)
                    hits += bool(rel)
                assert ev.top_k_map(list(q), qlabels, dataset, labels, _Enc(), k=k, allowed=allowed) == float(np.mean(aps)), (kind, k)
                assert ev.top_k_accuracy(list(q), qlabels, dataset, labels, _Enc(), k=k, allowed=allowed) == hits / 6, (kind, k)
            with pytest.raises(ValueError, match="k=None is not built"):
                ev.top_k_map(list(q), qlabels, dataset, labels, _Enc(), allowed=allowed)
            if isinstance(allowed, Subset):
                allowed.close()
    stale = indexes["dense"].subset(ids)
    with pytest.raises(ValueError, match="another index"):
        ev.retrieve_top_k_similar(q[0], indexes["int8"], _Enc(), k=2, allowed=stale)
    stale.close()
