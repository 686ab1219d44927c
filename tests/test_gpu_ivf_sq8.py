"""GPU tests of the inverted lists over the int8 code rows (csrc/ivf_sq8.hip, pvsim/ivf_int8.py) against the NumPy twin
(tests/ivf_sq8_numpy.py).  The dot product of two code rows is an integer and every other step is a single float32 operation, so
every comparison is on bytes: np.array_equal on the indices, bit patterns on the scores."""
import numpy as np
import pytest

import ivf_sq8_numpy as tw
import sq8_numpy as sq

pytestmark = pytest.mark.gpu


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _code_rows(nq, N, L):
    """the asymmetric integer rows of tests/test_gpu_sq8.py: Q[i][t] and X[j][t] follow different patterns; planted duplicates (exact
    ties, decided by the id) and, where 127^2 L exceeds 2^24, two rows whose sums with query 0 differ by one and collapse to one float"""
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


def _cent_rows(nlist, L):
    """centroid code rows of a third pattern"""
    ld = sq.ld_of(L)
    t = np.arange(L, dtype=np.int64)[None, :]
    c = np.arange(nlist, dtype=np.int64)[:, None]
    cc = np.zeros((nlist, ld), np.int8)
    cc[:, :L] = (13 * c + 7 * t + (c * t) % 7) % 251 - 125
    return cc, sq.factors(cc)


class _Stored:
    """rows in (list, original index) order on the device, with the host arrays the twin reads"""

    def __init__(self, ctx, dc, idb, lists, nlist):
        self.ids, self.list_off = tw.sort_into_lists(lists, nlist)
        self.codes, self.inv, self.nlist = dc[self.ids], idb[self.ids], nlist
        self.bufs = [_up(ctx, a) for a in (self.codes, self.inv, self.ids, self.list_off)]

    def free(self):
        for b in self.bufs:
            b.free()


def _scan(ctx, d_qc, d_iq, nq, L, probe, st, k, slice_rows=0):
    """the entry point on uploaded probes -> (idx, val); the outputs are pre-filled and carry a guard row behind them"""
    d_probe = _up(ctx, probe)
    d_idx, d_val = ctx.buffer((nq + 1) * k * 8).fill_bytes(0x5A), ctx.buffer((nq + 1) * k * 4).fill_bytes(0x5A)
    ctx.ivf_sq8_scan_topk_dev(d_qc.ptr, d_iq.ptr, nq, L, d_probe.ptr, probe.shape[1], st.bufs[3].ptr, st.list_off, st.nlist,
                              st.bufs[0].ptr, st.bufs[1].ptr, st.bufs[2].ptr, k, d_idx.ptr, d_val.ptr, slice_rows=slice_rows)
    idx, val = d_idx.download((nq + 1, k), np.int64), d_val.download((nq + 1, k), np.float32)
    assert (idx[nq:].view(np.uint8) == 0x5A).all() and (val[nq:].view(np.uint8) == 0x5A).all()      # nothing past row nq
    for b in (d_probe, d_idx, d_val):
        b.free()
    return idx[:nq], val[:nq]


def _want(flat, probe, st):
    """the twin's candidate rows (tw.candidate_rows) read out of the flat score matrix (original order); tw.select ranks them"""
    nq, nprobe = probe.shape
    W = tw.width(st.list_off, nprobe)
    cval, cid = np.full((nq, W), -np.inf, np.float32), np.full((nq, W), -1, np.int32)
    for q in range(nq):
        rows = [np.arange(st.list_off[l], st.list_off[l + 1]) for l in probe[q] if 0 <= l < st.nlist]
        rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
        cval[q, :rows.size], cid[q, :rows.size] = flat[q, st.ids[rows]], st.ids[rows]
    return cval, cid


# ------------------------------------------------------------------------------------------------ entry point against the twin
@pytest.mark.parametrize("nq", [1, 3, 17])
@pytest.mark.parametrize("L", [1, 64, 65, 1000, 4100])
def test_scan_matches_twin(gpu_ctx, L, nq):
    """Large candidate rows first, small ones after them in the same workspace block: a slot the second call failed to write would
    hold a live score and id of the first."""
    for N in (1000, 300, 127, 1):
        qc, iq, dc, idb = _code_rows(nq, N, L)
        flat = sq.scores(qc, iq, dc, idb)
        d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
        for nlist in (64, 7, 2, 1):
            cc, ci = _cent_rows(nlist, L)
            st = _Stored(gpu_ctx, dc, idb, tw.assign(dc, idb, cc, ci), nlist)
            if nlist == 64:
                assert (np.diff(st.list_off) == 0).any()                         # empty lists exist (and nlist > N at N = 1)
            for nprobe in sorted({1, min(2, nlist), nlist}, reverse=True):
                probe = tw.probes(qc, iq, cc, ci, nprobe)
                cval, cid = _want(flat, probe, st)
                if (N, nlist) == (127, 7):                                       # the helper is the twin's candidate row
                    tv, ti = tw.candidate_rows(qc, iq, probe, st.list_off, st.codes, st.inv, st.ids)
                    assert np.array_equal(ti, cid) and _same_bits(tv, cval)
                for k in sorted({1, 16, 17, min(N, 100)}):
                    want_i, want_v = tw.select(cval, cid, k)
                    got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, k)
                    assert np.array_equal(got_i, want_i), (L, nq, N, nlist, nprobe, k, np.argwhere(got_i != want_i)[:4])
                    assert _same_bits(got_v, want_v), (L, nq, N, nlist, nprobe, k)
                    if nprobe == nlist:                                          # every row once: the flat lists, as far as k <= N
                        fi, fv = sq.topk(flat, min(k, N))
                        assert np.array_equal(got_i[:, :min(k, N)], fi) and _same_bits(got_v[:, :min(k, N)], fv)
            st.free()
        d_qc.free(), d_iq.free()


def test_stale_slots_of_an_earlier_call_are_not_read(gpu_ctx):
    """A first call with a wide candidate row (every list of 1000 rows), then calls whose rows are short or empty, in the same
    workspace block: padding must be written, not inherited."""
    nq, N, L, nlist = 3, 1000, 65, 7
    qc, iq, dc, idb = _code_rows(nq, N, L)
    flat = sq.scores(qc, iq, dc, idb)
    cc, ci = _cent_rows(nlist, L)
    wide = _Stored(gpu_ctx, dc, idb, tw.assign(dc, idb, cc, ci), nlist)
    lists = np.full(N, 3, np.int64)
    lists[:5] = 0                                                              # five rows in list 0, the rest in list 3, the others empty
    narrow = _Stored(gpu_ctx, dc, idb, lists, nlist)
    d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
    all_lists = np.tile(np.arange(nlist, dtype=np.int64), (nq, 1))
    got = _scan(gpu_ctx, d_qc, d_iq, nq, L, all_lists, wide, 100)
    want = tw.select(*_want(flat, all_lists, wide), 100)
    assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1])
    for probe in (np.array([[1, 2], [0, 1], [5, 6]], np.int64),                # empty + empty, five rows, empty + empty
                  np.array([[0], [1], [0]], np.int64)):
        got = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, narrow, 17)
        want = tw.select(*_want(flat, probe, narrow), 17)
        assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), probe
        assert (got[0][0 if probe.shape[1] == 2 else 1] == -1).all()
    for b in (d_qc, d_iq):
        b.free()
    wide.free(), narrow.free()


# ------------------------------------------------------------------------------------------------ slices
def test_slice_size_changes_nothing(gpu_ctx):
    """slice_rows 0, 16, 48, 4096: the same bytes.  The lists are set by hand: list 0 ends one slot before the seam at 16 and the
    one row of list 1 is the last slot of that slice; the one row of list 5 is the first slot of the slice at 160; list 3 is empty;
    the long lists are cut by seams of 16 and 48 inside them."""
    nq, N, L, nlist = 3, 300, 65, 7
    sizes = [15, 1, 40, 0, 104, 1, 139]
    assert sum(sizes) == N and sum(sizes[:1]) == 15 and sum(sizes[:5]) == 160
    qc, iq, dc, idb = _code_rows(nq, N, L)
    flat = sq.scores(qc, iq, dc, idb)
    lists = np.repeat(np.arange(nlist), sizes)[np.random.default_rng(1).permutation(N)]      # original indices spread over the lists
    st = _Stored(gpu_ctx, dc, idb, lists, nlist)
    d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
    plan = gpu_ctx.ivf_sq8_scan_plan(nq, nlist, st.list_off, nlist, 0)
    assert plan["W"] == 320 and plan["slice_rows"] % 16 == 0 and plan["slice_rows"] >= 64
    assert gpu_ctx.ivf_sq8_scan_plan(nq, nlist, st.list_off, nlist, 17) == dict(plan, slice_rows=32, slices=10)
    probes = [np.tile(np.arange(nlist, dtype=np.int64), (nq, 1)),
              np.array([[6, 5, 4, 3, 2, 1, 0], [1, 0, 5, 4, 2, 6, 3], [3, 1, 5, 0, 6, 2, 4]], np.int64),
              np.array([[1, 5, 0], [5, 1, 3], [4, 6, 1]], np.int64)]
    for probe in probes:
        for k in (1, 17, 100):
            want_i, want_v = tw.select(*_want(flat, probe, st), k)
            for slice_rows in (0, 16, 48, 4096):
                got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, k, slice_rows)
                assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), (probe.shape, k, slice_rows)
    for b in (d_qc, d_iq):
        b.free()
    st.free()


# ------------------------------------------------------------------------------------------------ short and empty candidate rows
def test_short_and_empty_candidate_rows(gpu_ctx):
    nq, N, L, nlist = 4, 127, 1000, 64
    qc, iq, dc, idb = _code_rows(nq, N, L)
    flat = sq.scores(qc, iq, dc, idb)
    lists = (np.arange(N) % 9) * 7                                             # nine lists of about 14 rows, 55 empty ones
    st = _Stored(gpu_ctx, dc, idb, lists, nlist)
    sizes = np.diff(st.list_off)
    assert sizes[1] == 0 and sizes[2] == 0 and sizes[0] == 15 and sizes[7] == 14
    d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
    probe = np.array([[1, 2, 3],                                               # all probed lists empty
                      [7, 1, 2],                                               # 14 live candidates, k = 17: three unfilled slots
                      [-1, 0, nlist],                                          # -1 and nlist count as empty lists
                      [0, 7, 14]], np.int64)
    for k in (1, 17, 100):
        want_i, want_v = tw.select(*_want(flat, probe, st), k)
        got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, k)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), k
        assert (got_i[0] == -1).all() and np.isneginf(got_v[0]).all()
        assert (got_i[1, :min(k, 14)] >= 0).all() and (got_i[1, 14:] == -1).all() and np.isneginf(got_v[1, 14:]).all()
        assert set(got_i[2, :min(k, 15)].tolist()) <= set(st.ids[:15].tolist()) and (got_i[2, 15:] == -1).all()
    # N = 0: only (-1, -inf); nq = 0: nothing is written
    empty = _Stored(gpu_ctx, dc[:0], idb[:0], np.zeros(0, np.int64), nlist)
    got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, empty, 5)
    assert (got_i == -1).all() and np.isneginf(got_v).all()
    gpu_ctx.ivf_sq8_scan_topk_dev(None, None, 0, L, None, 3, None, st.list_off, nlist, None, None, None, 5, None, None)
    for b in (d_qc, d_iq):
        b.free()
    st.free(), empty.free()


def test_entry_point_refuses_bad_arguments(gpu_ctx):
    nq, N, L, nlist = 2, 20, 65, 4
    qc, iq, dc, idb = _code_rows(nq, N, L)
    st = _Stored(gpu_ctx, dc, idb, np.arange(N) % nlist, nlist)
    d_qc, d_iq, d_probe = _up(gpu_ctx, qc), _up(gpu_ctx, iq), _up(gpu_ctx, np.array([[0, 1], [2, 3]], np.int64))
    d_idx, d_val = gpu_ctx.buffer(nq * 8 * 8), gpu_ctx.buffer(nq * 8 * 4)

    def call(L=L, nprobe=2, list_off=st.list_off, nlist=nlist, k=5, slice_rows=0, qcodes=d_qc.ptr, codes=st.bufs[0].ptr, nq=nq, idx=d_idx.ptr):
        gpu_ctx.ivf_sq8_scan_topk_dev(qcodes, d_iq.ptr, nq, L, d_probe.ptr, nprobe, st.bufs[3].ptr, list_off, nlist, codes, st.bufs[1].ptr,
                                      st.bufs[2].ptr, k, idx, d_val.ptr, slice_rows=slice_rows)

    call()
    broken, late = st.list_off.copy(), st.list_off.copy()
    broken[2] = broken[1] - 1
    late[0] = 1
    for kw in (dict(L=0), dict(L=131073), dict(nprobe=0), dict(nprobe=5), dict(k=0), dict(k=1025), dict(slice_rows=-1), dict(nq=-1),
               dict(list_off=broken), dict(list_off=late), dict(qcodes=d_qc.ptr + 8), dict(codes=st.bufs[0].ptr + 4), dict(qcodes=None),
               dict(codes=None), dict(idx=None)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        gpu_ctx.ivf_sq8_scan_topk_dev(d_qc.ptr, d_iq.ptr, nq, L, d_probe.ptr, 1, st.bufs[3].ptr, np.zeros(2, np.int64), 0, st.bufs[0].ptr,
                                      st.bufs[1].ptr, st.bufs[2].ptr, 1, d_idx.ptr, d_val.ptr)
    for b in (d_qc, d_iq, d_probe, d_idx, d_val):
        b.free()
    st.free()


# ------------------------------------------------------------------------------------------------ extremes
def test_largest_sum_and_one_row_per_list(gpu_ctx):
    L = sq.MAX_L
    signs = np.array([1, -1, 1, 1, -1, -1, 1, -1], np.int8)
    dc = (signs[:, None] * np.full((1, L), 127, np.int8)).astype(np.int8)       # 8 rows of +-127
    qc = np.full((1, L), 127, np.int8)
    a = sq.acc(qc, dc)[0]
    assert a[0] == 2114060288 and a[1] == -2114060288
    iq, idb = sq.factors(qc), sq.factors(dc)
    ones = np.ones(8, np.float32)
    flat, raw = sq.scores(qc, iq, dc, idb), sq.scores(qc, ones[:1], dc, ones)
    lists = (signs < 0).astype(np.int64)                                        # two lists: the positive rows, the negative rows
    d_qc, d_iq, d_one = _up(gpu_ctx, qc), _up(gpu_ctx, iq), _up(gpu_ctx, ones[:1])
    for probe in (np.array([[0, 1]], np.int64), np.array([[1, 0]], np.int64), np.array([[1]], np.int64)):
        st = _Stored(gpu_ctx, dc, idb, lists, 2)
        got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, 1, L, probe, st, 8)
        want_i, want_v = tw.select(*_want(flat, probe, st), 8)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v)
        st.free()
        st = _Stored(gpu_ctx, dc, ones, lists, 2)                              # factors of one: the converted sums themselves
        got_i, got_v = _scan(gpu_ctx, d_qc, d_one, 1, L, probe, st, 8)
        want_i, want_v = tw.select(*_want(raw, probe, st), 8)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v)
        if probe.shape[1] == 2:
            assert got_v[0, 0] == np.float32(2114060288) and got_v[0, 7] == np.float32(-2114060288) and got_i[0].tolist() == [0, 2, 3, 6, 1, 4, 5, 7]
        else:
            assert got_i[0].tolist() == [1, 4, 5, 7, -1, -1, -1, -1] and got_v[0, 0] == np.float32(-2114060288)
        st.free()
    for b in (d_qc, d_iq, d_one):
        b.free()
    # one row per list
    nq, N, L = 3, 40, 64
    qc, iq, dc, idb = _code_rows(nq, N, L)
    flat = sq.scores(qc, iq, dc, idb)
    st = _Stored(gpu_ctx, dc, idb, np.random.default_rng(2).permutation(N), N)
    d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
    for nprobe in (1, 5, N):
        probe = np.stack([np.random.default_rng(3 + r).permutation(N)[:nprobe] for r in range(nq)]).astype(np.int64)
        got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, 16)
        want_i, want_v = tw.select(*_want(flat, probe, st), 16)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), nprobe
    for b in (d_qc, d_iq):
        b.free()
    st.free()


# ------------------------------------------------------------------------------------------------ class level
def _blobs(rng, n, L, centres):
    return (centres[rng.integers(0, len(centres), n)] + 0.3 * rng.standard_normal((n, L))).astype(np.float32)


def _map(x, first=0):
    return {f"img/{first + i:04d}.png": x[i] for i in range(x.shape[0])}


def _arrays_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3]))) and _same_bits(a[1], b[1])


def _assert_equals_fresh(index, survivors: dict, cent, q, ctx):
    """every array equals that of a fresh build from the survivors with the same centroids (and the twin's), and rank equals the twin"""
    import pvsim
    x = np.array(list(survivors.values()))
    got = index._download()
    assert index.keys() == list(survivors.keys()) and len(index) == len(survivors)
    want = tw.build(x, cent)
    assert np.array_equal(got[0], want["codes"]) and _same_bits(got[1], want["inv"])
    assert np.array_equal(got[2], want["ids"]) and np.array_equal(got[3], want["list_off"])
    assert np.array_equal(index.list_sizes, np.diff(want["list_off"]))
    fresh = pvsim.IVFInt8Index.build(survivors, cent, ctx)
    assert _arrays_equal(got, fresh._download())
    fresh.close()
    k = min(7, len(survivors))
    for nprobe in (1, index.nlist):
        got_i, got_v = index.rank(q, k, nprobe)
        want_i, want_v = tw.rank(q, x, cent, k, nprobe)
        assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), nprobe


def test_build_from_every_source_and_flat_equality(gpu_ctx):
    import pvsim
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((5, 70)).astype(np.float32)
    x, q = _blobs(rng, 60, 70, centres), _blobs(rng, 6, 70, centres)
    x[7] = x[3] * np.float32(4.0)                            # the scale cancels: an exact tie, decided by the id
    m = _map(x)
    dense, flat = DeviceIndex(m, gpu_ctx), pvsim.Int8Index(m, gpu_ctx)
    a = pvsim.IVFInt8Index.build(m, centres, gpu_ctx)
    b = pvsim.IVFInt8Index.build(dense, centres)
    c = pvsim.IVFInt8Index.build(flat, centres)
    assert _arrays_equal(a._download(), b._download()) and _arrays_equal(a._download(), c._download())
    assert np.array_equal(dense.matrix, x) and len(flat) == 60          # the sources are left as they are
    assert a.shape == (60, 70) and len(a) == 60 and a.paths == list(m) and a.keys() == list(m) and "img/0003.png" in a
    assert a.nlist == 5 and a.centroids is not None and np.array_equal(a.centroids, centres) and a.list_sizes.sum() == 60
    assert a.nbytes_breakdown == {"codes": 60 * 128, "factors": 240, "ids": 240, "list_off": 48, "centroid_codes": 5 * 128,
                                  "centroid_factors": 20}
    assert a.nbytes == flat.nbytes + 4 * 60 + 48 + 5 * 132 and a.modifications == 0
    _assert_equals_fresh(a, m, centres, q, gpu_ctx)
    for k in (1, 10, 60):                                    # every list probed: the flat index's lists, byte for byte
        got, want = a.rank(q, k, nprobe=5), flat.rank(q, k)
        assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), k
    pos = {int(i): p for p, i in enumerate(a.rank(x[3:4], 60, 5)[0][0])}
    assert pos[3] < pos[7]
    one = a.rank(q[:1], 10, 2, slice_rows=16)
    assert a.last_scan["slice_rows"] == 16 and a.last_scan["W"] % 64 == 0 and 0 < a.last_scan["candidates"] <= 60
    two = a.rank(q[:1], 10, 2)
    assert np.array_equal(one[0], two[0]) and _same_bits(one[1], two[1]) and a.last_scan["slice_rows"] >= 64
    # the error cases
    assert a.rank(q[:0], 3, 1)[0].shape == (0, 3)
    with pytest.raises(TypeError, match="float64"):
        a.rank(q.astype(np.float64), 3, 1)
    for k, nprobe in ((0, 1), (61, 1), (3, 0), (3, 6), (3, None)):
        with pytest.raises(ValueError):
            a.rank(q, k, nprobe)
    with pytest.raises(ValueError):
        a.rank(q[:, :69], 3, 1)
    bad = q.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        a.rank(bad, 3, 1)
    with pytest.raises(TypeError):
        pvsim.IVFInt8Index.build(DeviceIndex({p: v.astype(np.float64) for p, v in m.items()}, gpu_ctx), centres)
    with pytest.raises(TypeError, match="float64"):
        pvsim.IVFInt8Index.build(m, centres.astype(np.float64), gpu_ctx)
    with pytest.raises(ValueError):
        pvsim.IVFInt8Index.build(m, centres[:, :69], gpu_ctx)
    with pytest.raises(TypeError, match="float32 rows to train on"):
        pvsim.IVFInt8Index.fit(flat, 3)
    for nlist, train in ((0, None), (61, None), (5, 4), (5, 61), (2.5, None)):
        with pytest.raises(ValueError):
            pvsim.IVFInt8Index.fit(m, nlist, train=train, ctx=gpu_ctx)
    # N = 1 and one row per list
    single = pvsim.IVFInt8Index.build(_map(x[:1]), centres, gpu_ctx)
    got = single.rank(q, 1, 5)
    want = tw.rank(q, x[:1], centres, 1, 5)
    assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]) and (got[0] == 0).all()
    each = pvsim.IVFInt8Index.build(_map(x[:5]), x[:5].copy(), gpu_ctx)
    assert each.list_sizes.tolist() == [1, 1, 1, 1, 1] and each.rank(x[:5], 1, 1)[0][:, 0].tolist() == [0, 1, 2, 3, 4]
    for ix in (a, b, c, dense, flat, single, each):
        ix.close()


def test_fit_is_deterministic_and_equals_the_twin(gpu_ctx):
    import pvsim
    from pvsim.index import DeviceIndex
    from pvsim.ivf_int8 import _draw
    from pvsim.learn import _rng
    rng = np.random.default_rng(9)
    n, nt, L, nlist = 260, 200, 64, 5
    centres = rng.standard_normal((4, L)).astype(np.float32)
    x = _blobs(rng, n, L, centres)
    m = _map(x)
    a = pvsim.IVFInt8Index.fit(m, nlist, train=nt, random_state=3, ctx=gpu_ctx)
    dense = DeviceIndex(m, gpu_ctx)
    b = pvsim.IVFInt8Index.fit(dense, nlist, train=nt, random_state=3)
    assert _arrays_equal(a._download(), b._download()) and _same_bits(a.centroids, b.centroids)
    c = pvsim.IVFInt8Index.build(m, a.centroids, gpu_ctx)
    assert _arrays_equal(a._download(), c._download())
    # the twin's training on the same sample, the same initial rows and the device's own inverse norms
    sample, init = _draw(n, nt, nlist, _rng(3))
    assert sample.size == nt and (np.diff(sample) > 0).all() and len(set(init.tolist())) == nlist
    want = tw.train(x[sample], dense.inv_norms[sample], init, max_iter=10)
    assert _same_bits(a.centroids, want)
    cc = a._cent_codes.download((nlist, sq.ld_of(L)), np.int8)
    ci = a._cent_inv.download((nlist,), np.float32)
    want_cc, want_ci = sq.encode(want)
    assert np.array_equal(cc, want_cc) and _same_bits(ci, want_ci)
    one = pvsim.IVFInt8Index.fit(m, nlist, train=nt, random_state=3, max_iter=1, ctx=gpu_ctx)
    assert _same_bits(one.centroids, tw.train(x[sample], dense.inv_norms[sample], init, max_iter=1))
    every = pvsim.IVFInt8Index.fit(m, nlist, random_state=4, ctx=gpu_ctx)      # train=None: every row is a training row
    s_all, i_all = _draw(n, None, nlist, _rng(4))
    assert np.array_equal(s_all, np.arange(n)) and _same_bits(every.centroids, tw.train(x, dense.inv_norms, i_all, max_iter=10))
    for ix in (a, b, c, one, every, dense):
        ix.close()


def test_updates_equal_a_fresh_build(gpu_ctx):
    import pvsim
    from pvsim.index import DeviceIndex
    rng = np.random.default_rng(6)
    L = 65
    centres = rng.standard_normal((4, L)).astype(np.float32)
    cent = np.concatenate([centres, -centres.sum(axis=0, keepdims=True)]).astype(np.float32)      # list 4 attracts no blob row
    x, q = _blobs(rng, 40, L, centres), _blobs(rng, 5, L, centres)
    live = _map(x[:20])
    index = pvsim.IVFInt8Index.build(live, cent, gpu_ctx)
    assert index.list_sizes[4] == 0
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)

    new = _map(x[20:26], 20)                                 # add 6
    index.add(new)
    live.update(new)
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)

    first, last = list(live)[0], list(live)[-1]              # remove 2: the first and the last
    index.remove([last, first])
    del live[first], live[last]
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)

    middle = list(live)[len(live) // 2]                      # del one
    del index[middle]
    del live[middle]
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)

    new = {"img/empty-list.png": cent[4].copy()}             # add into the empty list
    index.add(new)
    live.update(new)
    assert index.list_sizes[4] == 1
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)

    keys = list(live)                                         # remove a whole list
    stored = index._download()
    big = int(np.argmax(index.list_sizes))
    members = stored[2][stored[3][big]:stored[3][big + 1]]
    index.remove([keys[i] for i in members])
    for i in members:
        del live[keys[i]]
    assert index.list_sizes[big] == 0
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)

    more = _map(x[26:40], 26)                                # resident rows are read in place
    dense = DeviceIndex(more, gpu_ctx)
    index.add(dense)
    live.update(more)
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)
    dense.close()
    assert index.modifications == 6

    index.reserve(1000)                                      # nothing to grow: the arrays stay
    _assert_equals_fresh(index, live, cent, q, gpu_ctx)
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
        index.add({"img/new.png": np.full(L, np.inf, np.float32)})
    with pytest.raises(ValueError):
        index.reserve(-1)
    assert _arrays_equal(before, index._download()) and index.keys() == list(live) and index.modifications == 6
    index.close()


def test_save_and_load(gpu_ctx, tmp_path):
    import pvsim
    rng = np.random.default_rng(7)
    centres = rng.standard_normal((6, 100)).astype(np.float32)
    x, q = _blobs(rng, 50, 100, centres), _blobs(rng, 4, 100, centres)
    index = pvsim.IVFInt8Index.build(_map(x), centres, gpu_ctx)
    fn = str(tmp_path / "ivf8.npz")
    index.save(fn)
    with np.load(fn, allow_pickle=False) as z:
        assert z["codes"].shape == (50, 100) and z["codes"].dtype == np.int8 and str(z["kind"]) == "ivf_int8_index"
    back = pvsim.IVFInt8Index.load(fn, gpu_ctx)
    assert _arrays_equal(index._download(), back._download()) and back.keys() == index.keys() and back.shape == (50, 100)
    assert _same_bits(back.centroids, centres)
    cc = [ix._cent_codes.download((6, 128), np.int8) for ix in (index, back)]
    assert np.array_equal(cc[0], cc[1])
    for nprobe in (1, 3, 6):
        a, b = index.rank(q, 9, nprobe), back.rank(q, 9, nprobe)
        assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1])
    back.add({"img/extra.png": x[0] * np.float32(2)})        # a loaded index is updated like a built one
    assert len(back) == 51 and back.rank(x[:1], 2, 6)[0][0].tolist() == [0, 50]
    with pytest.raises(ValueError):
        pvsim.Int8Index.load(fn, gpu_ctx)
    with pytest.raises(ValueError):
        pvsim.IVFCompactIndex.load(fn, gpu_ctx)
    flat = pvsim.Int8Index(_map(x), gpu_ctx)
    flat_fn = str(tmp_path / "flat.npz")
    flat.save(flat_fn)
    with pytest.raises(ValueError, match="not an IVF int8 index file"):
        pvsim.IVFInt8Index.load(flat_fn, gpu_ctx)
    index.close(), back.close(), flat.close()


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
    cent = vecs[[0, 6, 12, 18]].copy()
    index = pvsim.IVFInt8Index.build(dict(zip(paths, vecs)), cent, gpu_ctx)
    query = images[11]
    qv = enc.encode(query).reshape(1, -1).astype(np.float32)
    for nprobe in (1, 4):
        want_i, want_v = tw.rank(qv, vecs, cent, 5, nprobe)
        hits = ev.retrieve_top_k_similar(query, index, enc, k=5, nprobe=nprobe)
        live = want_i[0] >= 0
        assert [p for p, _ in hits][:int(live.sum())] == [paths[i] for i in want_i[0][live]] and hits[0][0] == paths[11]
        assert [np.float32(s) for _, s in hits][:int(live.sum())] == want_v[0][live].tolist()
    labels = {p: i % 5 for i, p in enumerate(paths)}
    assert ev.top_k_accuracy(images[:6], [i % 5 for i in range(6)], index, labels, enc, k=1, nprobe=1) == 1.0
    assert ev.top_k_map(images[:6], [i % 5 for i in range(6)], index, labels, enc, k=25, nprobe=4) > 0
    with pytest.raises(ValueError, match="pass nprobe="):
        ev.retrieve_top_k_similar(query, index, enc, k=5)
    with pytest.raises(ValueError, match="k=None on an IVFInt8Index is not built"):
        ev.top_k_map(images[:2], [0, 1], index, labels, enc, k=None, nprobe=2)
    for kw in (dict(expand=pvsim.QueryExpansion()), dict(rerank=10), dict(diffuse=object()), dict(reciprocal=object()), dict(allowed=[0, 1])):
        with pytest.raises(ValueError, match=next(iter(kw)) + "= on an IVFInt8Index is not built"):
            ev.retrieve_top_k_similar(query, index, enc, k=5, nprobe=2, **kw)
    index.close()
