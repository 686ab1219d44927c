"""GPU tests of the inverted lists of the compact index (csrc/ivf.hip, pvsim.IVFCompactIndex): every kernel against the NumPy twin
(tests/ivf_numpy.py), bit for bit -- include/pvsim.h fixes each summation order, so there is no tolerance to argue about."""
import ctypes as C

import numpy as np
import pytest

import ivf_numpy as iv
import pq_numpy as tw

pytestmark = pytest.mark.gpu

ASSIGN_LDS_FLOATS = 16384      # centroid floats one LDS chunk of the assignment kernel holds


def _up(ctx, a):
    a = np.ascontiguousarray(a)
    return ctx.buffer(max(a.nbytes, 16)).upload(a)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ assignment + residual
@pytest.mark.parametrize("n,d,nlist", [(1, 2, 1), (65, 64, 7), (1000, 257, 300), (1000, 2, 7), (65, 257, 1), (1, 64, 300)])
def test_assign_and_residual_match_twin(gpu_ctx, n, d, nlist):
    """values spanning 2^-6 .. 2^6; centroid 1 is repeated as the last one (its list must stay empty: the lowest l keeps a tie),
    a third of the rows sit exactly on centroids.  (1000, 257, 300) is 77100 centroid floats: five LDS chunks."""
    rng = np.random.default_rng(1000 + n + d + nlist)
    cent = (rng.standard_normal((nlist, d)) * np.exp2(rng.integers(-6, 7, (nlist, 1)))).astype(np.float32)
    if nlist >= 3:
        cent[nlist - 1] = cent[1]
    x = (cent[rng.integers(0, nlist, n)] * (1 + 0.3 * rng.standard_normal((n, d)))).astype(np.float32)
    x[::3] = cent[rng.integers(0, nlist, len(x[::3]))]
    if nlist >= 3:
        x[0] = cent[nlist - 1]
    d_x, d_c, d_l, d_r = _up(gpu_ctx, x), _up(gpu_ctx, cent), gpu_ctx.buffer(n * 4), gpu_ctx.buffer(n * d * 4)
    gpu_ctx.ivf_assign_dev(d_x.ptr, n, d, d_c.ptr, nlist, d_l.ptr, d_r.ptr)
    lists, res = d_l.download((n,), np.int32), d_r.download((n, d), np.float32)
    want_l, want_r = iv.assign(x, cent)
    assert np.array_equal(lists, want_l) and np.array_equal(_bits(res), _bits(want_r))
    if nlist >= 3:
        assert lists[0] == 1 and not (lists == nlist - 1).any()
    if (n, d, nlist) == (1000, 257, 300):
        assert nlist * d > ASSIGN_LDS_FLOATS
        gpu_ctx.ivf_assign_dev(d_x.ptr, n, d, d_c.ptr, nlist, d_l.ptr, None)          # labels alone
        assert np.array_equal(d_l.download((n,), np.int32), want_l)
    for b in (d_x, d_c, d_l, d_r):
        b.free()


@pytest.mark.parametrize("n,d,nlist", [(65, 64, 7), (1000, 5, 255)])
def test_assignment_and_coarse_terms_equal_a_one_subspace_quantiser(gpu_ctx, n, d, nlist):
    """one nearest-codeword kernel and one table kernel serve both entry points: the labels of pvs_ivf_assign_dev are the codes of
    pvs_pq_encode_dev for the quantiser m = 1, ksub = nlist, dsub = d built from the same centroids, the coarse terms are its
    table, and the residual is x - c[label], one float32 subtraction per element.  Centroid 1 is repeated as the last one."""
    rng = np.random.default_rng(1050 + n)
    cent = (rng.standard_normal((1, nlist, d)) * np.exp2(rng.integers(-20, 21, (1, nlist, 1)))).astype(np.float32)
    cent[:, nlist - 1] = cent[:, 1]
    x = cent[0][rng.integers(0, nlist, n)]
    noisy = rng.random(n) < 0.5
    x[noisy] *= (1 + 0.3 * rng.standard_normal((int(noisy.sum()), d))).astype(np.float32)
    x[0] = cent[0, nlist - 1]
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    table = gpu_ctx.pq(cent)
    d_x, d_c, d_q = _up(gpu_ctx, x), _up(gpu_ctx, cent[0]), _up(gpu_ctx, q)
    d_l, d_r, d_codes = gpu_ctx.buffer(n * 4), gpu_ctx.buffer(n * d * 4), gpu_ctx.buffer(max(n, 16))
    d_co, d_lut = gpu_ctx.buffer(3 * nlist * 4), gpu_ctx.buffer(3 * nlist * 4)
    gpu_ctx.ivf_assign_dev(d_x.ptr, n, d, d_c.ptr, nlist, d_l.ptr, d_r.ptr)
    gpu_ctx.pq_encode_dev(table, d_x.ptr, n, d_codes.ptr)
    gpu_ctx.ivf_coarse_dev(d_q.ptr, 3, d, d_c.ptr, nlist, d_co.ptr)
    gpu_ctx.pq_lut_dev(table, d_q.ptr, 3, d_lut.ptr)
    labels, codes = d_l.download((n,), np.int32), d_codes.download((n,), np.uint8)
    assert np.array_equal(labels, codes.astype(np.int32))
    assert np.array_equal(labels, iv.assign(x, cent[0])[0]) and labels[0] == 1 and not (labels == nlist - 1).any()
    assert np.array_equal(d_co.download((3, nlist), np.float32).view(np.uint32), d_lut.download((3, nlist), np.float32).view(np.uint32))
    assert np.array_equal(_bits(d_r.download((n, d), np.float32)), _bits(x - cent[0][labels]))
    table.close()
    for b in (d_x, d_c, d_q, d_l, d_r, d_codes, d_co, d_lut):
        b.free()


# ------------------------------------------------------------------------------------------------ coarse terms, probes
@pytest.mark.parametrize("nq,d,nlist", [(3, 2, 1000), (2, 3, 65536)])
def test_coarse_terms_beyond_one_block_per_subspace(gpu_ctx, nq, d, nlist):
    """the table kernel splits a sub-space's entries over blocks of 256: 1000 entries are four blocks with a ragged last one,
    65536 (the limit of nlist) are 256 blocks"""
    rng = np.random.default_rng(1150 + nq)
    cent = (rng.standard_normal((nlist, d)) * np.exp2(rng.integers(-6, 7, (nlist, 1)))).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    d_q, d_c, d_o = _up(gpu_ctx, q), _up(gpu_ctx, cent), gpu_ctx.buffer(nq * nlist * 4 + 16).fill_bytes(0x5A)
    gpu_ctx.ivf_coarse_dev(d_q.ptr, nq, d, d_c.ptr, nlist, d_o.ptr)
    got = d_o.download((nq * nlist + 4,), np.float32)
    assert np.array_equal(_bits(got[:-4].reshape(nq, nlist)), _bits(iv.coarse(q, cent)))
    assert (got[-4:].view(np.uint8) == 0x5A).all()
    for b in (d_q, d_c, d_o):
        b.free()


@pytest.mark.parametrize("nq,d,nlist", [(1, 2, 1), (5, 64, 7), (130, 257, 300)])
def test_coarse_terms_and_probes_match_twin(gpu_ctx, nq, d, nlist):
    rng = np.random.default_rng(1100 + nq)
    cent = (rng.standard_normal((nlist, d)) * np.exp2(rng.integers(-6, 7, (nlist, 1)))).astype(np.float32)
    if nlist >= 3:
        cent[nlist - 1] = cent[1]                                  # equal coarse terms: the lower list comes first
    q = rng.standard_normal((nq, d)).astype(np.float32)
    d_q, d_c, d_o = _up(gpu_ctx, q), _up(gpu_ctx, cent), gpu_ctx.buffer(nq * nlist * 4)
    gpu_ctx.ivf_coarse_dev(d_q.ptr, nq, d, d_c.ptr, nlist, d_o.ptr)
    co = d_o.download((nq, nlist), np.float32)
    want = iv.coarse(q, cent)
    assert np.array_equal(_bits(co), _bits(want))
    for nprobe in sorted({1, min(3, nlist), nlist}):
        d_i, d_v = gpu_ctx.buffer(nq * nprobe * 8), gpu_ctx.buffer(nq * nprobe * 4)
        gpu_ctx.topk_dev(d_o.ptr, nq, nlist, nlist, nprobe, 0, False, d_i.ptr, d_v.ptr)
        pi, pv = iv.probes(want, nprobe)
        assert np.array_equal(d_i.download((nq, nprobe), np.int64), pi)
        assert np.array_equal(_bits(d_v.download((nq, nprobe), np.float32)), _bits(pv))
        d_i.free(), d_v.free()
    for b in (d_q, d_c, d_o):
        b.free()


# ------------------------------------------------------------------------------------------------ scan + ranking
def _hand_lists(rng, N, nlist):
    """list of every row: list 0 holds more than half the rows, the last list (and list 2, if there are five) stays empty"""
    if nlist == 1:
        return np.zeros(N, np.int64)
    lists = rng.integers(0, nlist - 1, N)
    if nlist >= 5:
        lists[lists == 2] = 3
    lists[rng.random(N) < 0.55] = 0
    return lists


def _search(ctx, table, co, nprobe, off, ids, codes, inv_q, inv_db, k, code_offset=0):
    """the probes by pvs_topk_dev, then pvs_ivf_scan_topk_dev -> (idx, val); code_offset: the codes start that many bytes into
    their 16-byte aligned buffer (padded when not 0; otherwise the buffer ends at the last code)"""
    nq, m, ksub = table.shape
    nlist = co.shape[1]
    d_codes = ctx.buffer(codes.nbytes + 64).fill_bytes(0).upload(codes, offset=code_offset) if code_offset else _up(ctx, codes)
    bufs = [_up(ctx, table), _up(ctx, co), ctx.buffer(nq * nprobe * 8), ctx.buffer(nq * nprobe * 4), _up(ctx, off), d_codes,
            _up(ctx, ids), ctx.buffer(nq * k * 8), ctx.buffer(nq * k * 4)]
    assert bufs[5].ptr % 16 == 0
    d_t, d_co, d_pi, d_pv, d_off, d_codes, d_ids, d_idx, d_val = bufs
    d_iq = _up(ctx, inv_q) if inv_q is not None else None
    d_id = _up(ctx, inv_db) if inv_db is not None else None
    ctx.topk_dev(d_co.ptr, nq, nlist, nlist, nprobe, 0, False, d_pi.ptr, d_pv.ptr)
    ctx.ivf_scan_topk_dev(d_t.ptr, nq, m, ksub, d_pi.ptr, d_pv.ptr, nprobe, d_off.ptr, off, nlist, d_codes.ptr + code_offset, d_ids.ptr,
                          d_iq.ptr if d_iq else None, d_id.ptr if d_id else None, k, d_idx.ptr, d_val.ptr)
    out = d_idx.download((nq, k), np.int64), d_val.download((nq, k), np.float32)
    for b in bufs + [d_iq, d_id]:
        if b is not None:
            b.free()
    return out


def _scan_case(seed, nq, m, ksub, N, nlist):
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((nq, m, ksub)) * np.exp2(rng.integers(-3, 4, (nq, m, 1)))).astype(np.float32)
    co = rng.standard_normal((nq, nlist)).astype(np.float32)
    ids, off = iv.sort_into_lists(_hand_lists(rng, N, nlist), nlist)
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    inv_q = (0.5 + rng.random(nq)).astype(np.float32)
    inv_db = (0.5 + rng.random(N)).astype(np.float32)
    return table, co, off, ids, codes, inv_q, inv_db


def _check(ctx, case, nprobe, k, code_offset=0):
    table, co, off, ids, codes, inv_q, inv_db = case
    gi, gv = _search(ctx, table, co, nprobe, off, ids, codes, inv_q, inv_db, k, code_offset)
    wi, wv = iv.search(table, co, nprobe, off, ids, codes, inv_q, inv_db, k)
    assert np.array_equal(gi, wi), (nprobe, k)
    assert np.array_equal(_bits(gv), _bits(wv)), (nprobe, k)
    return gi


@pytest.mark.parametrize("N,nlist,m,ksub,nq", [(1, 1, 8, 16, 3), (65, 7, 6, 255, 5), (4099, 7, 16, 256, 4), (4099, 64, 7, 64, 9),
                                               (65, 64, 32, 256, 2), (4099, 1, 64, 256, 2)])
def test_scan_and_ranking_match_twin(gpu_ctx, N, nlist, m, ksub, nq):
    """hand-set lists (one holds more than half the rows, at least one is empty when nlist > 1); m = 8 takes the dword path, 6 and 7
    the byte path, 16 / 32 / 64 the 16-byte path; 4099 rows in one list cross a tile of the scan kernel"""
    case = _scan_case(1200 + N + nlist, nq, m, ksub, N, nlist)
    off = case[2]
    if nlist > 1:
        assert (np.diff(off) == 0).any() and np.diff(off).max() > N // 2
    short = False
    for nprobe in sorted({1, min(3, nlist), nlist}):
        for k in (1, 10, 100):
            gi = _check(gpu_ctx, case, nprobe, k)
            short = short or bool((gi == -1).any())
    assert short or N >= 4099                                      # k greater than the number of probed rows occurred


@pytest.mark.parametrize("code_offset", [0, 4, 1])
def test_scan_with_a_code_base_that_is_not_aligned(gpu_ctx, code_offset):
    """m = 16 with the codes 0, 4 and 1 bytes into their buffer: the twin's lists at every offset, whichever load width the host
    picks from the pointer.  The width itself (16, 4, 1 bytes) cannot be seen from here, a misaligned load returns the same
    bytes; csrc/bench/scan_plan_check.cpp pins it"""
    case = _scan_case(1250, 3, 16, 256, 65, 7)
    for nprobe in (1, 3, 7):
        for k in (1, 10, 100):
            _check(gpu_ctx, case, nprobe, k, code_offset)


def test_scan_queries_cross_the_query_block(gpu_ctx):
    """the candidate workspace holds 64 MiB: with 16448 slots per query (8 bytes each) a block is 510 queries, 600 queries are two"""
    N, nlist, m, ksub, nq = 16400, 2, 4, 16, 600
    rng = np.random.default_rng(1300)
    table = rng.standard_normal((nq, m, ksub)).astype(np.float32)
    co = rng.standard_normal((nq, nlist)).astype(np.float32)
    lists = np.zeros(N, np.int64)
    lists[::41] = 1
    ids, off = iv.sort_into_lists(lists, nlist)
    width = -(-int(np.diff(off).sum()) // 64) * 64
    assert (64 << 20) // (8 * width) < nq
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    inv_db = (0.5 + rng.random(N)).astype(np.float32)
    _check(gpu_ctx, (table, co, off, ids, codes, None, inv_db), 2, 10)


def test_scan_above_the_lds_segment_limit(gpu_ctx):
    """(m, ksub) = (161, 256): 41216 table entries, more than one LDS segment; the running sum lives across the segments"""
    case = _scan_case(1400, 3, 161, 256, 2500, 7)
    _check(gpu_ctx, case, 3, 10)
    _check(gpu_ctx, case, 7, 100)


def test_equal_scores_across_lists_rank_by_original_index(gpu_ctx):
    """integer tables and coarse terms: all sums exact.  Every row of lists 0 and 1 scores the same, so the cut at k falls inside
    a run of equal scores that spans two lists, and the order is by original index, not by stored position."""
    rng = np.random.default_rng(1500)
    N, nlist, m, ksub, nq = 300, 4, 4, 8, 3
    table = rng.integers(-2, 3, (nq, m, ksub)).astype(np.float32)
    table[0] = 1.0                                                 # query 0: the score is the coarse term + 4
    co = rng.integers(-1, 2, (nq, nlist)).astype(np.float32)
    co[0] = [3.0, 3.0, 5.0, -1.0]
    lists = rng.integers(0, 2, N)                                  # lists 0 and 1 interleave in the original order
    lists[:10] = [1, 0, 1, 1, 0, 1, 0, 0, 1, 0]
    lists[20:24] = 2                                               # four better rows in list 2; list 3 is empty
    ids, off = iv.sort_into_lists(lists, nlist)
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    case = (table, co, off, ids, codes, None, None)
    for nprobe, k in ((3, 10), (4, 100), (2, 5)):
        gi = _check(gpu_ctx, case, nprobe, k)
        if nprobe >= 3:
            assert gi[0, :4].tolist() == [20, 21, 22, 23]
            want = [i for i in range(N) if lists[i] < 2][:k - 4]
            assert gi[0, 4:].tolist() == want and len({int(lists[i]) for i in want}) == 2


def test_zero_centroid_one_list_equals_the_flat_scan(gpu_ctx):
    """identity 1 on the device: nlist = 1, coarse term +0 -> the bits of pvs_pq_scan_topk_dev on the same codes"""
    rng = np.random.default_rng(1600)
    N, m, ksub, nq, d = 3000, 16, 256, 6, 32
    table = rng.standard_normal((nq, m, ksub)).astype(np.float32)
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    inv_q, inv_db = (0.5 + rng.random(nq)).astype(np.float32), (0.5 + rng.random(N)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    d_q, d_c, d_o = _up(gpu_ctx, q), _up(gpu_ctx, np.zeros((1, d), np.float32)), gpu_ctx.buffer(nq * 4)
    gpu_ctx.ivf_coarse_dev(d_q.ptr, nq, d, d_c.ptr, 1, d_o.ptr)
    co = d_o.download((nq, 1), np.float32)
    assert not _bits(co).any()                                     # +0
    off, ids = np.array([0, N], np.int64), np.arange(N, dtype=np.int32)
    for k in (1, 10, 100):
        gi, gv = _search(gpu_ctx, table, co, 1, off, ids, codes, inv_q, inv_db, k)
        bufs = [_up(gpu_ctx, a) for a in (table, codes, inv_q, inv_db)] + [gpu_ctx.buffer(nq * k * 8), gpu_ctx.buffer(nq * k * 4)]
        gpu_ctx.pq_scan_topk_dev(bufs[0].ptr, nq, m, ksub, bufs[1].ptr, N, bufs[2].ptr, bufs[3].ptr, k, 0, False, bufs[4].ptr, bufs[5].ptr)
        fi, fv = bufs[4].download((nq, k), np.int64), bufs[5].download((nq, k), np.float32)
        assert np.array_equal(gi, fi) and np.array_equal(_bits(gv), _bits(fv))
        for b in bufs:
            b.free()
    for b in (d_q, d_c, d_o):
        b.free()


# ------------------------------------------------------------------------------------------------ paths no case above reaches
def _case_with_lists(seed, nq, m, ksub, lists, nlist):
    """_scan_case with the list of every row given"""
    rng = np.random.default_rng(seed)
    N = len(lists)
    table = (rng.standard_normal((nq, m, ksub)) * np.exp2(rng.integers(-3, 4, (nq, m, 1)))).astype(np.float32)
    co = rng.standard_normal((nq, nlist)).astype(np.float32)
    ids, off = iv.sort_into_lists(lists, nlist)
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    inv_q = (0.5 + rng.random(nq)).astype(np.float32)
    inv_db = (0.5 + rng.random(N)).astype(np.float32)
    return table, co, off, ids, codes, inv_q, inv_db


@pytest.mark.parametrize("nprobe", [128, 129, 301, 1024])
def test_many_probes(gpu_ctx, nprobe):
    """nlist = 1100: two probes per lane reach the second wave of the prefix scan at 129 probes, 1024 is the limit.  More than half
    the lists are empty (runs of empty probes in the binary search over the prefix sums), one list holds more than half the rows."""
    rng = np.random.default_rng(1800)
    N, nlist = 3000, 1100
    lists = rng.choice(rng.permutation(nlist)[:500], N)
    lists[rng.random(N) < 0.55] = lists[0]
    case = _case_with_lists(1801, 3, 4, 16, lists, nlist)
    sizes = np.diff(case[2])
    assert (sizes == 0).sum() > nlist // 2 and sizes.max() > N // 2
    for k in (10, 1024):
        _check(gpu_ctx, case, nprobe, k)


@pytest.mark.parametrize("m,ksub", [(160, 256), (148, 256), (372, 100)])
def test_more_than_one_lds_segment_on_each_load_width(gpu_ctx, m, ksub):
    """36864 table entries fit one LDS segment.  (160, 256): 16-byte code loads, segments of 144 and 16 sub-spaces; (148, 256): dword
    loads, 144 and 4; (372, 100): dword loads, 368 and 4, a segment length that is no power of two.  2200 of the 2500 rows sit in
    one list: the candidate row of a query that probes it is wider than one tile of 2048 slots and is served by two workgroups."""
    seg_m = 36864 // ksub
    assert m > seg_m and (m % 16 == 0 and seg_m % 16 == 0) == ((m, ksub) == (160, 256)) and m % 4 == 0 and seg_m % 4 == 0
    rng = np.random.default_rng(1900 + m)
    N, nlist = 2500, 7
    lists = rng.integers(1, nlist - 1, N)
    lists[rng.permutation(N)[:2200]] = 0
    case = _case_with_lists(1901 + m, 3, m, ksub, lists, nlist)
    case[1][0, 0], case[1][1, 0] = 9.0, -9.0                      # query 0 probes the long list first, query 1 last
    assert np.diff(case[2]).max() == 2200 > 2048
    for nprobe in (1, 3):
        for k in (10, 100):
            _check(gpu_ctx, case, nprobe, k)


def test_list_mode_ranking_across_chunks_at_depth(gpu_ctx):
    """9000 candidates per query are two 8192-slot chunks of the list-mode ranking, with a running list of k = 1000 / 1024 between
    them; with one probe, query 0 gets the list of 500 rows: fewer than k"""
    rng = np.random.default_rng(2000)
    N, nlist = 9000, 2
    lists = np.zeros(N, np.int64)
    lists[rng.permutation(N)[:500]] = 1
    case = _case_with_lists(2001, 3, 4, 16, lists, nlist)
    case[1][0], case[1][1] = [-1.0, 1.0], [1.0, -1.0]             # query 0 prefers list 1 (500 rows), query 1 list 0
    for k in (1000, 1024):
        gi = _check(gpu_ctx, case, 2, k)
        assert (gi >= 0).all()
    gi = _check(gpu_ctx, case, 1, 1000)
    assert (gi[0, :500] >= 0).all() and (gi[0, 500:] == -1).all() and (gi[1] >= 0).all()


def test_zero_and_nan_scores_come_back_in_canonical_form(gpu_ctx):
    """integer tables, all sums exact and <= 0.  Query 0: rows whose codes all pick a -0.0 entry under a -0.0 coarse term score
    -0.0, rows that pick the +0.0 entry score +0.0; they tie, rank by original index and come back as +0.0.  Query 1: one table
    entry is a NaN with sign and payload, another is -inf: NaN rows rank after the -inf rows and before the unfilled slots, and
    come back as the canonical quiet NaN."""
    rng = np.random.default_rng(2100)
    N, nlist, m, ksub, nq = 600, 3, 4, 4, 2
    table = np.empty((nq, m, ksub), np.float32)
    table[:] = [-0.0, -0.0, -1.0, -2.0]
    table[0, 0, 0] = 0.0
    table[1, 2, 3] = -np.inf
    table[1, 1, 2] = np.nan
    table[1].reshape(-1).view(np.uint32)[1 * ksub + 2] = 0xffc00123
    co = np.array([[-0.0, -0.0, -1.0], [-0.0, -1.0, -0.0]], np.float32)
    ids, off = iv.sort_into_lists(rng.integers(0, 2, N), nlist)   # list 2 is empty
    codes = rng.integers(0, ksub, (N, m)).astype(np.uint8)
    case = (table, co, off, ids, codes, None, None)
    exact = tw.scores(table, codes)                               # stored order
    s0 = np.full(N, -0.0, np.float32)                             # query 0: the coarse term of lists 0 and 1 is -0.0
    for s in range(m):
        s0 = s0 + table[0, s][codes[:, s]]
    zero = s0 == 0
    assert (zero & np.signbit(s0)).sum() >= 3 and (zero & ~np.signbit(s0)).sum() >= 3
    assert np.isnan(exact[1]).sum() > 100 and np.isneginf(exact[1]).sum() > 50
    for nprobe, k in ((2, 10), (2, 600), (3, 700), (1, 5)):
        gi, gv = _search(gpu_ctx, *case[:2], nprobe, *case[2:], k)
        wi, wv = iv.search(*case[:2], nprobe, *case[2:], k)
        assert np.array_equal(gi, wi) and np.array_equal(_bits(gv), _bits(wv)), (nprobe, k)
        assert not (_bits(gv) == 0x80000000).any() and (_bits(gv)[np.isnan(gv)] == 0x7fc00000).all()
        if nprobe == 2 and k == 10:
            assert not _bits(gv[0]).any()                        # ten zeros, all +0.0
            both = np.sort(ids[zero].astype(np.int64))[:10]
            assert gi[0].tolist() == both.tolist()
        if k >= 600:
            nan, ninf, unfilled = np.isnan(gv[1]), np.isneginf(gv[1]) & (gi[1] >= 0), gi[1] == -1
            assert nan.any() and ninf.any() and (k == 600 or unfilled.any())
            assert np.flatnonzero(ninf).max() < np.flatnonzero(nan).min()
            assert not unfilled.any() or np.flatnonzero(nan).max() < np.flatnonzero(unfilled).min()


# ------------------------------------------------------------------------------------------------ through the class
@pytest.fixture(scope="module")
def corpus():
    """400 VLAD-like rows of L = 256 (sparse blocks, signed, L2-normalised) and 10 queries near rows 0, 40, ..."""
    rng = np.random.default_rng(1700)
    basis = rng.standard_normal((16, 256)) * (rng.random((16, 256)) < 0.3)
    x = rng.standard_normal((400, 16)) @ basis + 0.2 * rng.standard_normal((400, 256))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = (x[::40] + 0.05 * rng.standard_normal((10, 256))).astype(np.float32)
    return x, q


FIT = dict(m=8, n_components=32, ksub=32, keep_projected=True, random_state=5, max_iter=10)


@pytest.fixture(scope="module")
def fitted(gpu_ctx, corpus):
    from pvsim import IVFCompactIndex
    x, q = corpus
    db = {f"img/{i:04d}.jpg": x[i] for i in range(len(x))}
    index = IVFCompactIndex.fit(db, 12, ctx=gpu_ctx, **FIT)
    yield index, db
    index.close()


def _twin_of(index, x, q):
    """the twin fed with the device's own projection, centroids and codebooks -> what rank must give"""
    codes, inv_db, proj = index._download()
    y = index.project(x)
    assert np.array_equal(_bits(proj), _bits(y))                   # kept rows stay in original order
    lists, res = iv.assign(y, index.centroids)
    ids, off = iv.sort_into_lists(lists, index.nlist)
    assert np.array_equal(ids, index._ids) and np.array_equal(off, index._list_off)
    assert np.array_equal(index.list_sizes, np.bincount(lists, minlength=index.nlist))
    cb = index.quantizer.codebooks
    assert np.array_equal(codes, tw.encode(res, cb)[ids])
    yq = index.project(q)
    ctx = index.context
    d_y, d_i = _up(ctx, yq), ctx.buffer(len(yq) * 4)
    ctx.row_inv_norms_dev(d_y.ptr, len(yq), yq.shape[1], d_i.ptr)
    inv_q = d_i.download((len(yq),), np.float32)
    d_y.free(), d_i.free()
    d_p, d_n = _up(ctx, y), ctx.buffer(len(y) * 4)
    ctx.row_inv_norms_dev(d_p.ptr, len(y), y.shape[1], d_n.ptr)
    inv_orig = d_n.download((len(y),), np.float32)
    d_p.free(), d_n.free()
    assert np.array_equal(_bits(inv_db), _bits(inv_orig[ids]))     # norms in stored order
    return dict(table=tw.lut(yq, cb), co=iv.coarse(yq, index.centroids), off=off, ids=ids, codes=codes, inv_q=inv_q, inv_db=inv_db,
                inv_orig=inv_orig, y=y, yq=yq)


def test_fit_and_rank_equal_the_twin(fitted, corpus):
    index, _ = fitted
    x, q = corpus
    t = _twin_of(index, x, q)
    assert index.nlist == 12 and index.list_sizes.sum() == 400 and len(index) == 400
    for nprobe in (1, 3, 12):
        idx, val = index.rank(q, 10, nprobe)
        wi, wv = iv.search(t["table"], t["co"], nprobe, t["off"], t["ids"], t["codes"], t["inv_q"], t["inv_db"], 10)
        assert np.array_equal(idx, wi) and np.array_equal(_bits(val), _bits(wv))
        ridx, rval = index.rank(q, 10, nprobe, rerank=50)
        cand, _ = iv.search(t["table"], t["co"], nprobe, t["off"], t["ids"], t["codes"], t["inv_q"], t["inv_db"], 50)
        wi, wv = tw.rerank(cand, tw.rescore(t["yq"], t["y"], cand, t["inv_q"], t["inv_orig"]), 10)
        assert np.array_equal(ridx, wi) and np.array_equal(_bits(rval), _bits(wv))
        filled = (cand >= 0).sum(1)
        for r in range(len(q)):                                    # unfilled slots stay last
            assert (ridx[r, :min(10, filled[r])] >= 0).all() and (ridx[r, filled[r]:] == -1).all()
    ridx, _ = index.rank(q, 10, 12, rerank=50)
    assert np.array_equal(ridx[:, 0], np.arange(0, 400, 40))       # every list probed + exact re-ranking: the source row comes first


def test_save_load_eval_and_device_index_source(gpu_ctx, fitted, corpus, tmp_path):
    from pvsim import IVFCompactIndex
    from pvsim import eval as ev
    from pvsim.index import DeviceIndex
    index, db = fitted
    x, q = corpus
    fn = str(tmp_path / "ivf.npz")
    index.save(fn)
    back = IVFCompactIndex.load(fn, ctx=gpu_ctx)
    assert back.paths == index.paths and back.nbytes == index.nbytes and np.array_equal(back.list_sizes, index.list_sizes)
    dev = DeviceIndex(db, gpu_ctx)
    other = IVFCompactIndex.fit(dev, 12, **FIT)
    assert other.context is gpu_ctx and np.array_equal(other.centroids, index.centroids)
    for got, want in zip(other._download(), index._download()):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    for rr in (0, 30):
        a = index.rank(q, 10, 3, rerank=rr)
        for o in (back, other):
            b = o.rank(q, 10, 3, rerank=rr)
            assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    back.close(), other.close(), dev.close()

    class Identity:
        def encode(self, v):
            return v

    idx, val = index.rank(q[:1], 5, 2)
    hits = ev.retrieve_top_k_similar(q[0], index, Identity(), k=5, nprobe=2)
    keep = idx[0] >= 0
    assert [p for p, _ in hits] == [index.paths[i] for i in idx[0][keep]] and [s for _, s in hits] == val[0][keep].tolist()
    ridx, _ = index.rank(q[:1], 5, 2, rerank=20)
    hits = ev.retrieve_top_k_similar(q[0], index, Identity(), k=5, rerank=20, nprobe=2)
    assert [p for p, _ in hits] == [index.paths[i] for i in ridx[0] if i >= 0]
    labels = {p: i // 40 for i, p in enumerate(index.paths)}
    assert ev.top_k_accuracy(list(q), list(range(10)), index, labels, Identity(), k=20, nprobe=12) > 0.9
    assert 0.0 <= ev.top_k_map(list(q), list(range(10)), index, labels, Identity(), k=20, nprobe=1, rerank=20) <= 1.0
    # one probed list holds fewer than k rows: the unfilled slots are dropped from the returned list
    full, _ = index.rank(q[:1], 400, 1)
    got = ev.retrieve_top_k_similar(q[0], index, Identity(), k=400, nprobe=1)
    assert len(got) == int((full[0] >= 0).sum()) < 400


def test_fit_frees_its_buffers_when_it_fails(gpu_ctx, fitted, monkeypatch):
    from pvsim import IVFCompactIndex
    _, db = fitted
    taken = []
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
        IVFCompactIndex.fit(db, 12, ctx=gpu_ctx, **FIT)
    import gc
    gc.collect()
    assert taken and all(b.ptr == 0 for b in taken)                # every buffer the call took was given back


# ------------------------------------------------------------------------------------------------ error paths
def test_invalid_arguments_return_an_error_without_a_launch(gpu_ctx):
    from pvsim import _ffi
    lib, h = _ffi.lib(), gpu_ctx.handle
    buf = gpu_ctx.buffer(1 << 16).fill_bytes(0)
    p = buf.ptr
    vp, null = C.c_void_p, C.c_void_p(None)
    off = np.array([0, 20, 20, 50], np.int64)
    buf.upload(off, offset=32768)

    def scan(lut=p, nq=2, m=4, ksub=16, probe=p + 4096, pval=p + 8192, nprobe=2, d_off=p + 32768, h_off=off, nlist=3, codes=p + 12288,
             ids=p + 16384, k=5, idx=p + 20480, val=p + 24576):
        return lib.pvs_ivf_scan_topk_dev(h, vp(lut), nq, m, ksub, vp(probe), vp(pval), nprobe, vp(d_off),
                                         _ffi.ptr(h_off) if h_off is not None else null, nlist, vp(codes), vp(ids), null, null, k, vp(idx),
                                         vp(val))

    assert scan() == _ffi.PVS_OK
    bad_off = np.array([0, 30, 20, 50], np.int64)
    huge = np.array([0, 1 << 31, 1 << 31, 1 << 31], np.int64)
    for bad in (dict(m=0), dict(ksub=257), dict(ksub=0), dict(k=0), dict(k=1025), dict(nprobe=0), dict(nprobe=4), dict(nlist=0),
                dict(nlist=65537), dict(idx=None), dict(val=None), dict(idx=p + 4), dict(val=p + 2), dict(lut=None), dict(codes=None),
                dict(ids=None), dict(probe=None), dict(pval=None), dict(d_off=None), dict(h_off=None), dict(h_off=bad_off),
                dict(h_off=huge), dict(nq=-1), dict(probe=p + 4100)):
        assert scan(**bad) == _ffi.PVS_ERR_INVALID, bad
        assert lib.pvs_last_error()
    assert scan(nq=0, idx=None, val=None) == _ffi.PVS_OK               # nq == 0 is a no-op
    wide = np.arange(1027, dtype=np.int64)                             # nlist = 1026, one row per list: the limit is 1024 probes
    assert scan(nprobe=1025, nlist=1026, h_off=wide) == _ffi.PVS_ERR_INVALID and lib.pvs_last_error()

    def assign(x=p, n=5, d=4, cent=p + 4096, nlist=3, lst=p + 8192, res=p + 12288):
        return lib.pvs_ivf_assign_dev(h, vp(x), n, d, vp(cent), nlist, vp(lst), vp(res))

    assert assign() == _ffi.PVS_OK and assign(res=None) == _ffi.PVS_OK and assign(n=0, x=None) == _ffi.PVS_OK
    for bad in (dict(d=0), dict(nlist=0), dict(nlist=65537), dict(n=-1), dict(n=1 << 31), dict(x=None), dict(cent=None), dict(lst=None),
                dict(x=p + 2), dict(lst=p + 8194)):
        assert assign(**bad) == _ffi.PVS_ERR_INVALID, bad
    assert assign(d=16385) == _ffi.PVS_ERR_UNSUPPORTED

    def coarse(q=p, nq=5, d=4, cent=p + 4096, nlist=3, out=p + 8192):
        return lib.pvs_ivf_coarse_dev(h, vp(q), nq, d, vp(cent), nlist, vp(out))

    assert coarse() == _ffi.PVS_OK and coarse(nq=0, q=None) == _ffi.PVS_OK
    for bad in (dict(d=0), dict(nlist=0), dict(nlist=65537), dict(nq=-1), dict(q=None), dict(cent=None), dict(out=None), dict(out=p + 1)):
        assert coarse(**bad) == _ffi.PVS_ERR_INVALID, bad
    gpu_ctx.sync()
    buf.free()
