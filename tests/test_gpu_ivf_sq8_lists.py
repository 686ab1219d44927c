"""GPU tests of the probed int8 scan by list (csrc/ivf_sq8.hip): pvs_ivf_sq8_group_probes_dev against its NumPy
twin (tests/ivf_sq8_lists_numpy.py) and pvs_ivf_sq8_scan_lists_topk_dev against the scan by query (pvs_ivf_sq8_scan_topk_dev) and the
twin of section 26 (tests/ivf_sq8_numpy.py).  The dot product of two code rows is an integer and every other step is a single float32
operation, so every comparison is on bytes: np.array_equal on the indices, bit patterns on the scores.  The integer row patterns are
those of tests/test_gpu_ivf_sq8.py, restated."""
import functools

import numpy as np
import pytest

import ivf_sq8_lists_numpy as lt
import ivf_sq8_numpy as tw
import sq8_numpy as sq

pytestmark = pytest.mark.gpu


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _code_rows(nq, N, L):
    """asymmetric integer rows: Q[i][t] and X[j][t] follow different patterns; planted duplicates (exact ties, decided by the id) and,
    where 127^2 L exceeds 2^24, two rows whose sums with query 0 differ by one and collapse to one float"""
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


def _scan(ctx, d_qc, d_iq, nq, L, probe, st, k, lists=True, query_block=0):
    """the scan by list (or, lists=False, the scan by query) on uploaded probes -> (idx, val); the outputs are pre-filled with 0x5A and
    carry a guard row behind them"""
    d_probe = _up(ctx, probe)
    d_idx, d_val = ctx.buffer((nq + 1) * k * 8).fill_bytes(0x5A), ctx.buffer((nq + 1) * k * 4).fill_bytes(0x5A)
    args = (d_qc.ptr, d_iq.ptr, nq, L, d_probe.ptr, probe.shape[1], st.bufs[3].ptr, st.list_off, st.nlist, st.bufs[0].ptr, st.bufs[1].ptr,
            st.bufs[2].ptr, k, d_idx.ptr, d_val.ptr)
    if lists:
        ctx.ivf_sq8_scan_lists_topk_dev(*args, query_block=query_block)
    else:
        ctx.ivf_sq8_scan_topk_dev(*args)
    idx, val = d_idx.download((nq + 1, k), np.int64), d_val.download((nq + 1, k), np.float32)
    assert (idx[nq:].view(np.uint8) == 0x5A).all() and (val[nq:].view(np.uint8) == 0x5A).all()      # nothing past row nq
    for b in (d_probe, d_idx, d_val):
        b.free()
    return idx[:nq], val[:nq]


def _want(flat, probe, st):
    """the candidate rows of section 26 read out of the flat score matrix (original order); tw.select ranks them"""
    nq, nprobe = probe.shape
    W = tw.width(st.list_off, nprobe)
    cval, cid = np.full((nq, W), -np.inf, np.float32), np.full((nq, W), -1, np.int32)
    for q in range(nq):
        rows = [np.arange(st.list_off[l], st.list_off[l + 1]) for l in probe[q] if 0 <= l < st.nlist]
        rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
        cval[q, :rows.size], cid[q, :rows.size] = flat[q, st.ids[rows]], st.ids[rows]
    return cval, cid


# ------------------------------------------------------------------------------------------------ 1. the grouping against the twin
def _ragged_offsets(rng, nlist, N):
    """N rows over nlist lists, about a third of the lists empty; nlist > N leaves most of them empty"""
    lists = rng.integers(0, nlist, N)
    lists[lists % 3 == 1] = 0
    return tw.sort_into_lists(lists, nlist)[1]


@pytest.mark.parametrize("nlist", [1, 7, 64, 300])
@pytest.mark.parametrize("nq", [1, 3, 130])
def test_grouping_equals_the_twin(gpu_ctx, nq, nlist):
    rng = np.random.default_rng(1000 * nq + nlist)
    for N in (40, 700):                                                        # nlist = 64 and 300 exceed N = 40
        list_off = _ragged_offsets(rng, nlist, N)
        assert list_off[-1] == N and (nlist < 7 or (np.diff(list_off) == 0).any())
        d_off = _up(gpu_ctx, list_off)
        for nprobe in sorted({1, min(2, nlist), nlist}):
            probe = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)
            for bad in (-1, nlist):                                            # probes outside [0, nlist): empty lists, no pair
                probe[rng.integers(0, nq), rng.integers(0, nprobe)] = bad
            base, total, goff, gq, gbase = lt.group_probes(probe, list_off)
            P = int(goff[nlist])
            assert P == int(((probe >= 0) & (probe < nlist)).sum()) and gq.size == P
            d_probe = _up(gpu_ctx, probe)
            outs = [gpu_ctx.buffer(max(4 * n, 16)).fill_bytes(0x5A) for n in (nq * nprobe, nq, nlist + 1, nq * nprobe, nq * nprobe)]
            gpu_ctx.ivf_sq8_group_probes_dev(d_probe.ptr, nq, nprobe, d_off.ptr, nlist, *(o.ptr for o in outs))
            got = [o.download((n,), np.int32) for o, n in zip(outs, (nq * nprobe, nq, nlist + 1, nq * nprobe, nq * nprobe))]
            case = (nq, nlist, N, nprobe)
            assert np.array_equal(got[0].reshape(nq, nprobe), base) and np.array_equal(got[1], total), case
            assert np.array_equal(got[2], goff), case
            assert np.array_equal(got[3][:P], gq) and np.array_equal(got[4][:P], gbase), case
            assert (got[3][P:].view(np.uint8) == 0x5A).all() and (got[4][P:].view(np.uint8) == 0x5A).all(), case      # nothing behind the pairs
            for b in [d_probe] + outs:
                b.free()
        d_off.free()


# ------------------------------------------------------------------------------------------------ 2. the scan against the old entry and the twin
# planted list lengths: a 1-row list is followed by a long one, so the rows past its end in the tile are another list's live rows
PLANTED = ([1, 257, 0, 127, 1, 128, 129], [257, 1, 129, 0, 128, 1, 127])
N_PLANTED, NQ_MAX = 643, 257


@functools.lru_cache(maxsize=None)
def _fixture(L):
    """code rows, centroid rows and the flat score matrix for NQ_MAX queries: computed once per L, sliced by nq, never written"""
    qc, iq, dc, idb = _code_rows(NQ_MAX, N_PLANTED, L)
    cc, ci = _cent_rows(7, L)
    flat = tw.blas_scores(qc, iq, dc, idb)
    assert _same_bits(flat[:3, :50], sq.scores(qc[:3], iq[:3], dc[:50], idb[:50]))
    for a in (qc, iq, dc, idb, cc, ci, flat):
        a.setflags(write=False)
    return qc, iq, dc, idb, cc, ci, flat


@pytest.mark.parametrize("nq", [1, 3, 17, 130, 257])
@pytest.mark.parametrize("L", [1, 64, 65, 1000, 4100])
def test_scan_equals_the_scan_by_query_and_the_twin(gpu_ctx, L, nq):
    qc, iq, dc, idb, cc, ci, flat = _fixture(L)
    qc, iq, flat = qc[:nq], iq[:nq], flat[:nq]
    N, nlist = N_PLANTED, 7
    d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
    for order, sizes in enumerate(PLANTED):
        assert sum(sizes) == N and sorted(sizes) == [0, 1, 1, 127, 128, 129, 257]
        lists = np.repeat(np.arange(nlist), sizes)[np.random.default_rng(order).permutation(N)]     # original indices spread over the lists
        st = _Stored(gpu_ctx, dc, idb, lists, nlist)
        assert np.array_equal(np.diff(st.list_off), sizes)
        for nprobe in (nlist, 2, 1):
            probe = tw.probes(qc, iq, cc, ci, nprobe, tw.blas_scores)
            cval, cid = _want(flat, probe, st)
            if (L, nq, nprobe) == (65, 17, 2):                                   # the tiles of the twin fill the rows of section 26
                tv, ti = lt.candidate_rows(qc, iq, probe, st.list_off, st.codes, st.inv, st.ids)
                assert np.array_equal(ti, cid) and _same_bits(tv, cval)
            for k in (1, 16, 17, 100):
                want_i, want_v = tw.select(cval, cid, k)
                got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, k)
                old_i, old_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, k, lists=False)
                case = (L, nq, order, nprobe, k)
                assert np.array_equal(got_i, old_i) and _same_bits(got_v, old_v), (case, np.argwhere(got_i != old_i)[:4])
                assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), (case, np.argwhere(got_i != want_i)[:4])
                if nprobe == nlist:                                              # every row once: the flat lists
                    fi, fv = sq.topk(flat, k)
                    assert np.array_equal(got_i, fi) and _same_bits(got_v, fv), case
        st.free()
    d_qc.free(), d_iq.free()


# ------------------------------------------------------------------------------------------------ 3. stale slots
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
                  np.array([[0], [1], [0]], np.int64),
                  np.array([[-1, 0, nlist], [1, 2, 4], [nlist, -1, 5]], np.int64)):
        got = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, narrow, 17)
        want = tw.select(*_want(flat, probe, narrow), 17)
        assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), probe
        assert (got[0][0 if probe.shape[1] == 2 else 1] == -1).all()
    # N = 0: only (-1, -inf); nq = 0: nothing is written
    empty = _Stored(gpu_ctx, dc[:0], idb[:0], np.zeros(0, np.int64), nlist)
    got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, all_lists, empty, 5)
    assert (got_i == -1).all() and np.isneginf(got_v).all()
    gpu_ctx.ivf_sq8_scan_lists_topk_dev(None, None, 0, L, None, 3, None, narrow.list_off, nlist, None, None, None, 5, None, None)
    for b in (d_qc, d_iq):
        b.free()
    wide.free(), narrow.free(), empty.free()


# ------------------------------------------------------------------------------------------------ 4. the query block
def test_query_block_changes_nothing(gpu_ctx):
    L, nq, nlist = 65, 257, 7
    qc, iq, dc, idb, cc, ci, flat = _fixture(L)
    lists = np.repeat(np.arange(nlist), PLANTED[0])[np.random.default_rng(0).permutation(N_PLANTED)]
    st = _Stored(gpu_ctx, dc, idb, lists, nlist)
    d_qc, d_iq = _up(gpu_ctx, qc), _up(gpu_ctx, iq)
    plan = gpu_ctx.ivf_sq8_scan_lists_plan(nq, nlist, st.list_off, nlist, 0)
    assert plan == {"W": 704, "query_block": 257, "row_tiles": 9, "pairs": 257 * 7}                  # 643 -> 704; tiles 1 + 3 + 0 + 1 + 1 + 1 + 2
    assert gpu_ctx.ivf_sq8_scan_lists_plan(nq, 2, st.list_off, nlist, 127) == {"W": 448, "query_block": 127, "row_tiles": 9, "pairs": 254}
    for nprobe in (nlist, 2):
        probe = tw.probes(qc, iq, cc, ci, nprobe, tw.blas_scores)
        want_i, want_v = tw.select(*_want(flat, probe, st), 17)
        for query_block in (1, 2, 127, 128, 0):
            got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, 17, query_block=query_block)
            assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v), (nprobe, query_block)
    for b in (d_qc, d_iq):
        b.free()
    st.free()


# ------------------------------------------------------------------------------------------------ 5. collapse and the largest sum
def test_collapsed_pair_and_largest_sum(gpu_ctx):
    # two sums above 2^24 that differ by one and convert to the same float: the order is decided by the id
    L, nq, nlist = 4100, 3, 7
    qc, iq, dc, idb, cc, ci, flat = _fixture(L)
    lists = np.arange(N_PLANTED) % nlist
    lists[5], lists[9] = 6, 2                                                  # the pair in different lists, the larger id stored first
    st = _Stored(gpu_ctx, dc, idb, lists, nlist)
    d_qc, d_iq = _up(gpu_ctx, qc[:nq]), _up(gpu_ctx, iq[:nq])
    probe = np.tile(np.arange(nlist, dtype=np.int64), (nq, 1))
    got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, nq, L, probe, st, 100)
    want_i, want_v = sq.topk(flat[:nq], 100)
    assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v)
    pos = {int(i): p for p, i in enumerate(got_i[0])}
    assert pos[9] == pos[5] + 1 and got_v[0, pos[5]] == got_v[0, pos[9]]
    for b in (d_qc, d_iq):
        b.free()
    st.free()
    # the largest sums an int32 holds: rows of +-127 at L = 131072
    L = sq.MAX_L
    signs = np.array([1, -1, -1, 1], np.int8)
    dc = (signs[:, None] * np.full((1, L), 127, np.int8)).astype(np.int8)
    qc = np.stack([np.full(L, 127, np.int8), np.full(L, -127, np.int8)])
    a = sq.acc(qc, dc)
    assert a[0, 0] == 2114060288 and a[0, 1] == -2114060288 and a[1, 1] == 2114060288
    ones_q, ones_d = np.ones(2, np.float32), np.ones(4, np.float32)
    lists = (signs < 0).astype(np.int64)
    d_qc = _up(gpu_ctx, qc)
    for fq, fd in ((sq.factors(qc), sq.factors(dc)), (ones_q, ones_d)):        # the scores, then the converted sums themselves
        flat = sq.scores(qc, fq, dc, fd)
        d_iq = _up(gpu_ctx, fq)
        st = _Stored(gpu_ctx, dc, fd, lists, 2)
        for probe in (np.array([[0, 1], [1, 0]], np.int64), np.array([[1], [0]], np.int64)):
            got_i, got_v = _scan(gpu_ctx, d_qc, d_iq, 2, L, probe, st, 4)
            old_i, old_v = _scan(gpu_ctx, d_qc, d_iq, 2, L, probe, st, 4, lists=False)
            want_i, want_v = tw.select(*_want(flat, probe, st), 4)
            assert np.array_equal(got_i, want_i) and _same_bits(got_v, want_v) and np.array_equal(got_i, old_i) and _same_bits(got_v, old_v)
        if fq is ones_q:
            assert got_v[0, 0] == np.float32(-2114060288) and got_i[0].tolist() == [1, 2, -1, -1] and got_i[1].tolist() == [0, 3, -1, -1]
        d_iq.free(), st.free()
    d_qc.free()


# ------------------------------------------------------------------------------------------------ 6. bad arguments
def test_entry_points_refuse_bad_arguments(gpu_ctx):
    nq, N, L, nlist, k = 2, 20, 65, 4, 5
    qc, iq, dc, idb = _code_rows(nq, N, L)
    st = _Stored(gpu_ctx, dc, idb, np.arange(N) % nlist, nlist)
    d_qc, d_iq, d_probe = _up(gpu_ctx, qc), _up(gpu_ctx, iq), _up(gpu_ctx, np.array([[0, 1], [2, 3]], np.int64))
    d_idx, d_val = gpu_ctx.buffer(nq * 8 * 8), gpu_ctx.buffer(nq * 8 * 4)

    def call(L=L, nprobe=2, list_off=st.list_off, nlist=nlist, k=k, query_block=0, qcodes=d_qc.ptr, codes=st.bufs[0].ptr, nq=nq, idx=d_idx.ptr):
        gpu_ctx.ivf_sq8_scan_lists_topk_dev(qcodes, d_iq.ptr, nq, L, d_probe.ptr, nprobe, st.bufs[3].ptr, list_off, nlist, codes, st.bufs[1].ptr,
                                            st.bufs[2].ptr, k, idx, d_val.ptr, query_block=query_block)

    call()
    good = d_idx.download((nq, k), np.int64)
    assert (good >= 0).all()
    broken, late = st.list_off.copy(), st.list_off.copy()
    broken[2] = broken[1] - 1
    late[0] = 1
    for kw in (dict(L=0), dict(L=131073), dict(nprobe=0), dict(nprobe=5), dict(k=0), dict(k=1025), dict(query_block=-1), dict(nq=-1),
               dict(list_off=broken), dict(list_off=late), dict(qcodes=d_qc.ptr + 8), dict(codes=st.bufs[0].ptr + 4), dict(qcodes=None),
               dict(codes=None), dict(idx=None), dict(nlist=0, list_off=np.zeros(1, np.int64))):
        d_idx.fill_bytes(0x5A), d_val.fill_bytes(0x5A)
        with pytest.raises(ValueError):
            call(**kw)
        gpu_ctx.sync()                                                          # nothing was launched: the outputs hold the fill
        assert (d_idx.download((nq * 8,), np.int64).view(np.uint8) == 0x5A).all(), kw
        assert (d_val.download((nq * 8,), np.float32).view(np.uint8) == 0x5A).all(), kw
    outs = [gpu_ctx.buffer(64).fill_bytes(0x5A) for _ in range(5)]
    for kw in (dict(qn=-1), dict(qn=65536), dict(nprobe=0), dict(nprobe=5), dict(nlist=0), dict(nlist=65537), dict(qn=2048, nprobe=1024, nlist=1024)):
        a = dict(dict(qn=nq, nprobe=2, nlist=nlist), **kw)
        with pytest.raises(ValueError):
            gpu_ctx.ivf_sq8_group_probes_dev(d_probe.ptr, a["qn"], a["nprobe"], st.bufs[3].ptr, a["nlist"], *(o.ptr for o in outs))
    with pytest.raises(ValueError):
        gpu_ctx.ivf_sq8_group_probes_dev(None, nq, 2, st.bufs[3].ptr, nlist, *(o.ptr for o in outs))
    gpu_ctx.sync()
    assert all((o.download((16,), np.int32).view(np.uint8) == 0x5A).all() for o in outs)
    with pytest.raises(ValueError):
        gpu_ctx.ivf_sq8_scan_lists_plan(nq, 5, st.list_off, nlist, 0)
    with pytest.raises(ValueError):
        gpu_ctx.ivf_sq8_scan_lists_plan(nq, 2, st.list_off, nlist, -1)
    for b in [d_qc, d_iq, d_probe, d_idx, d_val] + outs:
        b.free()
    st.free()


# ------------------------------------------------------------------------------------------------ 7. class level
def _blobs(rng, n, L, centres):
    return (centres[rng.integers(0, len(centres), n)] + 0.3 * rng.standard_normal((n, L))).astype(np.float32)


def _map(x, first=0):
    return {f"img/{first + i:04d}.png": x[i] for i in range(x.shape[0])}


def test_rank_by_lists_equals_rank_by_queries(gpu_ctx):
    import pvsim
    rng = np.random.default_rng(15)
    L = 70
    centres = rng.standard_normal((5, L)).astype(np.float32)
    x, q = _blobs(rng, 400, L, centres), _blobs(rng, 140, L, centres)
    x[7] = x[3] * np.float32(4.0)                            # the scale cancels: an exact tie, decided by the id
    live = _map(x[:300])
    index = pvsim.IVFInt8Index.build(live, centres, gpu_ctx)

    def compare():
        n = len(index)
        for nprobe in (1, 2, 5):
            for k in (1, 17, min(n, 100)):
                a = index.rank(q, k, nprobe)
                keys = set(index.last_scan)
                b = index.rank(q, k, nprobe, scan="lists")
                assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1]), (n, nprobe, k)
                assert keys == {"W", "slice_rows", "slices", "candidates"}       # a default call reports what it always did
                ls = index.last_scan
                assert set(ls) == {"scan", "W", "query_block", "row_tiles", "pairs", "candidates"} and ls["scan"] == "lists"
                assert ls["W"] % 64 == 0 and ls["query_block"] == 140 and ls["pairs"] == 140 * nprobe
                assert ls["row_tiles"] == int(((index.list_sizes + 127) // 128).sum())
        c = index.rank(q, 10, 2, scan="lists", query_block=33)
        d = index.rank(q, 10, 2, slice_rows=16)
        assert index.last_scan["slice_rows"] == 16 and np.array_equal(c[0], d[0]) and _same_bits(c[1], d[1])
        flat = pvsim.Int8Index(dict(zip(index.keys(), index_rows())), gpu_ctx)
        for k in (1, 10):                                    # every list probed: the flat index's lists, byte for byte
            got, want = index.rank(q, k, 5, scan="lists"), flat.rank(q, k)
            assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1]), k
        flat.close()

    rows = dict(live)

    def index_rows():
        return [rows[p] for p in index.keys()]

    compare()
    new = _map(x[300:], 300)
    index.add(new)
    rows.update(new)
    compare()
    gone = list(rows)[::3]
    index.remove(gone)
    for p in gone:
        del rows[p]
    compare()
    assert index.rank(q[:0], 3, 1, scan="lists")[0].shape == (0, 3)
    for kw in (dict(scan="auto"), dict(scan=None), dict(scan="lists", slice_rows=16), dict(query_block=4)):
        with pytest.raises(ValueError, match="scan|slice_rows|query_block"):
            index.rank(q, 3, 1, **kw)
    index.close()
