"""GPU tests of the ranking kernels (csrc/topk.hip) against the NumPy twin of their contract (tests/topk_numpy.py).

pvs_topk_dev and pvs_topk_merge_dev are called directly on the planted panels of tests/topk_cases.py -- nothing is computed before
the ranking -- under every kernel choice of PVS_OPT_TOPK_SELECT_ONLY (1 radix select, 2 rounds, 3 threshold filter, 0 the
launcher's own), and each run is compared with the twin: indices equal, values equal as bits.  No variant is compared with
another.  The float64 ranking has no entry of its own, so its scores are planted through the operands of pvs_cosine_topk_f64_dev.
Every output block sits between two sentinel rows that must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import topk_cases as tc
import topk_numpy as tk

pytestmark = pytest.mark.gpu

VARIANTS = (1, 2, 3, 0)
IDX_GUARD, VAL_GUARD = -7777, 1234.5


@pytest.fixture
def select(gpu_ctx):
    """sets PVS_OPT_TOPK_SELECT_ONLY; the option is back at 0 when the test ends, however it ends"""
    from pvsim import _ffi
    try:
        yield lambda v: gpu_ctx.set_option(_ffi.OPT_TOPK_SELECT_ONLY, int(v))
    finally:
        gpu_ctx.set_option(_ffi.OPT_TOPK_SELECT_ONLY, 0)


class _Lists:
    """device idx / val blocks of nq x k with one sentinel row in front and one behind"""

    def __init__(self, ctx, nq, k, vdt=np.float32):
        self.ctx, self.nq, self.k, self.vdt = ctx, nq, k, np.dtype(vdt)
        self.d_idx = ctx.buffer((nq + 2) * k * 8).upload(np.full((nq + 2, k), IDX_GUARD, np.int64))
        self.d_val = ctx.buffer((nq + 2) * k * self.vdt.itemsize).upload(np.full((nq + 2, k), VAL_GUARD, self.vdt))
        self.idx_ptr, self.val_ptr = self.d_idx.ptr + k * 8, self.d_val.ptr + k * self.vdt.itemsize

    def result(self):
        self.ctx.sync()
        idx, val = self.d_idx.download((self.nq + 2, self.k), np.int64), self.d_val.download((self.nq + 2, self.k), self.vdt)
        self.d_idx.free(), self.d_val.free()
        assert (idx[[0, -1]] == IDX_GUARD).all() and (val[[0, -1]] == self.vdt.type(VAL_GUARD)).all(), "a sentinel row was written"
        return idx[1:-1], val[1:-1]


def _same(got, want, what):
    gi, gv = got
    wi, wv = want
    if not np.array_equal(gi, wi):
        r, c = np.argwhere(gi != wi)[0]
        raise AssertionError(f"{what}: index [{r}][{c}] is {gi[r, c]}, the twin says {wi[r, c]}")
    gb, wb = tk.bits(gv), tk.bits(wv)
    if not np.array_equal(gb, wb):
        r, c = np.argwhere(gb != wb)[0]
        raise AssertionError(f"{what}: value [{r}][{c}] has bits {gb[r, c]:#x}, the twin says {wb[r, c]:#x}")


def _rank_panels(ctx, panels, offsets, k, pad=0, shift=0):
    """pvs_topk_dev on each panel in turn (merge from the second on) -> (idx, val).  pad: extra columns per row (ld = ncols + pad),
    filled with +inf so that a read past ncols would win; shift: bytes between a 256-byte boundary and the panel's first score"""
    nq = panels[0].shape[0]
    out = _Lists(ctx, nq, k)
    for p, (panel, off) in enumerate(zip(panels, offsets)):
        ncols = panel.shape[1]
        ld = ncols + pad
        host = tc.padded(panel, pad)
        buf = ctx.buffer(nq * ld * 4 + shift + 16)
        if host.size:
            buf.upload(host, offset=shift)
        assert buf.ptr % 256 == 0
        ctx.topk_dev(buf.ptr + shift, nq, ncols, ld, k, off, p > 0, out.idx_ptr, out.val_ptr)
        ctx.sync()
        buf.free()
    return out.result()


def _ks_for(ncols):
    for k in tc.KS + tc.KS_PAGED:
        n = tc.resolve_ncols(ncols, k)
        if n >= 0 and (k <= tc.KMAX or n > tc.KMAX):        # deeper than one launch only where the row has a second page
            yield n, k


# ------------------------------------------------------------------------------------------------ float32 panels
@pytest.mark.parametrize("group", sorted(tc.GROUPS))
@pytest.mark.parametrize("ncols", tc.NCOLS)
def test_panel_ranking_equals_the_twin(gpu_ctx, select, ncols, group):
    """every planted row kind at every k of the issue's list, under each kernel choice; k > 1024 pages"""
    for n, k in _ks_for(ncols):
        panel = tc.panel(group, n, k)
        want = tk.topk(panel, k)
        for v in VARIANTS:
            select(v)
            _same(_rank_panels(gpu_ctx, [panel], [0], k), want, f"ncols={n} k={k} variant={v}")


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("pad", [4, 3, 1])
@pytest.mark.parametrize("ncols", [63, 2049, 4099, 8197])
def test_row_stride_and_alignment(gpu_ctx, select, ncols, pad, shift):
    """ld > ncols with ld % 4 == 0 and != 0, the padding +inf; the panel starts on a 16-byte boundary or 4 bytes after one (the
    threshold filter then reads single floats even at ld % 4 == 0)"""
    for group in sorted(tc.GROUPS):
        for k in (1, 16, 17, 256):
            panel = tc.panel(group, ncols, k, seed=1)
            want = tk.topk(panel, k)
            assert not np.isposinf(want[1][[0, 2, 3]]).any()      # rows without +inf of their own: a padding column would show
            for v in VARIANTS:
                select(v)
                _same(_rank_panels(gpu_ctx, [panel], [0], k, pad=pad, shift=shift), want,
                      f"ncols={ncols} ld={ncols + pad} shift={shift} k={k} variant={v} group={group}")
    assert {(n + p) % 4 == 0 for n in (63, 2049, 4099, 8197) for p in (4, 3, 1)} == {True, False}


@pytest.mark.parametrize("ncols", [65, 4099])
def test_column_offset_at_the_32_bit_limit(gpu_ctx, select, ncols):
    """col_offset + ncols = 0xfffffffe is the last legal panel, one column more is PVS_ERR_UNSUPPORTED and writes nothing"""
    from pvsim import _ffi
    for end in (tc.INDEX_LIMIT, tc.INDEX_LIMIT - 1):
        off = end - ncols
        for k in (1, 16, 300):
            panel = tc.panel("A", ncols, k, seed=2)
            want = tk.topk(panel, k, off)
            assert want[0].max() == end - 1
            for v in VARIANTS:
                select(v)
                _same(_rank_panels(gpu_ctx, [panel], [off], k), want, f"end={end:#x} k={k} variant={v}")
    panel = tc.panel("A", ncols, 16, seed=2)
    buf = gpu_ctx.buffer(panel.nbytes).upload(panel)
    out = _Lists(gpu_ctx, panel.shape[0], 16)
    vp = C.c_void_p
    for v in VARIANTS:
        select(v)
        rc = _ffi.lib().pvs_topk_dev(gpu_ctx.handle, vp(buf.ptr), panel.shape[0], ncols, ncols, 16, tc.INDEX_LIMIT + 1 - ncols, 0,
                                     vp(out.idx_ptr), vp(out.val_ptr))
        assert rc == _ffi.PVS_ERR_UNSUPPORTED
    idx, val = out.result()
    assert (idx == IDX_GUARD).all() and (val == np.float32(VAL_GUARD)).all()
    buf.free()


# ------------------------------------------------------------------------------------------------ running-list merge
@pytest.mark.parametrize("k", [1, 2, 16, 17, 300, 1024])
@pytest.mark.parametrize("name", tc.MERGE_CASES)
def test_running_list_merge_equals_ranking_the_concatenation(gpu_ctx, select, name, k):
    """two and three panels of unequal size; the list after each panel is the ranking of what has arrived so far (an empty panel
    with merge = 1 therefore hands the sorted list back unchanged)"""
    panels, offs = tc.merge_case(name, k)
    for v in VARIANTS:
        select(v)
        for upto in range(1, len(panels) + 1):
            want = tk.merge_panels(panels[:upto], offs[:upto], k)
            _same(_rank_panels(gpu_ctx, panels[:upto], offs[:upto], k), want, f"{name} k={k} variant={v} after panel {upto}")


# ------------------------------------------------------------------------------------------------ paging
@pytest.mark.parametrize("ncols", tc.PAGING_NCOLS)
def test_paging_deeper_than_one_launch(gpu_ctx, select, ncols):
    """k > 1024: ties on a grid, rows whose numbers end exactly at, one before and one after a page boundary (the NaN that follows
    starts or ends a page), ncols between two pages: the last page is not full and the slots that remain are -1 / -inf"""
    rows = tc.paging_rows(ncols)
    for k in (1025, 2048, 2049):
        want = tk.topk(rows, k)
        assert (want[0][:, -1] == -1).all() == (ncols < k)
        for v in VARIANTS:
            select(v)
            _same(_rank_panels(gpu_ctx, [rows], [0], k), want, f"ncols={ncols} k={k} variant={v}")


# ------------------------------------------------------------------------------------------------ list mode
@pytest.mark.parametrize("k", [1, 16, 17, 1024])
@pytest.mark.parametrize("n_lists", [1, 2, 8, 9])
def test_merge_of_lists_equals_the_twin(gpu_ctx, select, n_lists, k):
    """pvs_topk_merge_dev: unfilled entries, a query without any entry, equal scores across lists, ids above 2^31"""
    idx_lists, val_lists = tc.merge_lists_case(n_lists, k)
    nq = idx_lists.shape[1]
    want = tk.merge_lists(idx_lists, val_lists, k)
    d_i, d_v = gpu_ctx.buffer(idx_lists.nbytes).upload(idx_lists), gpu_ctx.buffer(val_lists.nbytes).upload(val_lists)
    for v in VARIANTS:
        select(v)
        out = _Lists(gpu_ctx, nq, k)
        gpu_ctx.topk_merge_dev(d_i.ptr, d_v.ptr, n_lists, nq, k, out.idx_ptr, out.val_ptr)
        _same(out.result(), want, f"n_lists={n_lists} k={k} variant={v}")
    d_i.free(), d_v.free()


# ------------------------------------------------------------------------------------------------ float64 ranking
F64_NCOLS = (1, 1023, 1024, 2047, 2048, 2049, 8192, 8197, 16389)
SCALES = np.array([1.0, -1.0, 2.0])          # three queries [c, 0]: the row as planted, reversed, doubled


@pytest.mark.parametrize("group", sorted(tc.GROUPS))
@pytest.mark.parametrize("ncols", F64_NCOLS)
def test_float64_ranking_equals_the_twin(gpu_ctx, select, ncols, group):
    """L = 2, queries [c, 0] with c = 1, -1, 2, database rows [s, 0], no norm factors: the score is c s, exactly.  The device's own
    panel (pvs_cosine_f64_dev) is downloaded and must hold the planted products bit for bit where they are finite and not zero (a
    product of zero meets the +0 of the second term, so its sign is the sum's, not the plant's; there it must be a zero); that panel
    is ranked by the twin.  k crosses the wave kernel's condition (k <= 16, ncols >= 2048), the page (4096) and the chunk (8192)."""
    nq = len(SCALES)
    q = np.zeros((nq, 2))
    q[:, 0] = SCALES
    d_q = gpu_ctx.buffer(q.nbytes).upload(q)
    ks = sorted({k for k in (1, 16, 17, 4096, 4097, ncols) if k <= ncols})
    for k in ks:
        rows = tc.panel(group, ncols, k, np.float64, seed=3)
        for r, s in enumerate(rows):
            db = np.zeros((ncols, 2))
            db[:, 0] = s
            d_db, d_p = gpu_ctx.buffer(db.nbytes).upload(db), gpu_ctx.buffer(nq * ncols * 8)
            gpu_ctx.cosine_f64_dev(d_q.ptr, nq, d_db.ptr, ncols, 2, None, None, d_p.ptr, ncols)
            gpu_ctx.sync()
            panel = d_p.download((nq, ncols), np.float64)
            with np.errstate(over="ignore", invalid="ignore"):
                planted = SCALES[:, None] * s[None, :]
            exact = np.isfinite(planted) & (planted != 0)
            assert np.array_equal(tk.bits(panel)[exact], tk.bits(planted)[exact])
            assert (panel[planted == 0] == 0).all() and np.array_equal(np.isnan(panel), np.isnan(planted))
            assert np.array_equal(panel[np.isinf(planted)], planted[np.isinf(planted)])
            want = tk.topk(panel, k)
            for v in (1, 0):
                select(v)
                out = _Lists(gpu_ctx, nq, k, np.float64)
                gpu_ctx.cosine_topk_f64_dev(d_q.ptr, nq, d_db.ptr, ncols, 2, None, None, k, out.idx_ptr, out.val_ptr)
                _same(out.result(), want, f"f64 ncols={ncols} k={k} row={tc.GROUPS[group][r].__name__} option={v}")
            d_db.free(), d_p.free()
    d_q.free()
