"""NumPy twin of the ranking contract of csrc/topk.hip (include/pvsim.h, "top-k"), stated once for every search path:

  * rank by (score descending, global index ascending);
  * NaN comes after every number, -inf included;
  * -0 and +0 tie;
  * a zero score is returned as +0.0, any NaN as the canonical quiet NaN (0x7fc00000 / 0x7ff8000000000000);
  * slots that cannot be filled are idx = -1, val = -inf.

float32 or float64 scores; the returned values have the scores' dtype.  The same rule holds at any depth: the device reaches
k > 1024 by paging, this module just takes a longer prefix of one sorted row."""
import numpy as np

QNAN_BITS = {np.dtype(np.float32): 0x7fc00000, np.dtype(np.float64): 0x7ff8000000000000}
_UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def _float(a):
    a = np.asarray(a)
    assert a.dtype in QNAN_BITS, a.dtype
    return a


def qnan(dtype):
    """the canonical quiet NaN of `dtype` as a scalar of that dtype"""
    dt = np.dtype(dtype)
    return np.array([QNAN_BITS[dt]], _UINT[dt]).view(dt)[0]


def bits(a):
    """the values of a float32 / float64 array as unsigned integers (for bitwise comparisons)"""
    a = np.ascontiguousarray(_float(a))
    return a.view(_UINT[a.dtype])


def rank_row(ids, vals, k):
    """one row: ids int64 (n,), vals (n,) -> (idx int64 (k,), val (k,)); entries with id < 0 are skipped"""
    vals = _float(vals)
    ids = np.asarray(ids, np.int64)
    keep = ids >= 0
    ids, vals = ids[keep], vals[keep]
    nan = np.isnan(vals)
    zero = vals.dtype.type(0)
    number = np.where(nan, zero, vals) + zero                    # -0 + 0 = +0: equal scores tie and come back as +0
    order = np.lexsort((ids, -number, nan))[:k]                  # last key first: NaN flag, then score descending, then id
    idx = np.full(k, -1, np.int64)
    val = np.full(k, -np.inf, vals.dtype)
    idx[:len(order)] = ids[order]
    val[:len(order)] = np.where(nan[order], qnan(vals.dtype), number[order])
    return idx, val


def _rows(ids, vals, k):
    vals = _float(vals)
    out = [rank_row(ids[r], vals[r], k) for r in range(vals.shape[0])]
    idx = np.array([o[0] for o in out], np.int64).reshape(vals.shape[0], k)
    val = np.array([o[1] for o in out], vals.dtype).reshape(vals.shape[0], k)
    return idx, val


def topk(scores, k, col_offset=0):
    """scores (nq, ncols), column c has global index col_offset + c -> idx int64 (nq, k), val (nq, k)"""
    scores = _float(scores)
    nq, ncols = scores.shape
    ids = np.broadcast_to(np.arange(ncols, dtype=np.int64) + int(col_offset), (nq, ncols))
    return _rows(ids, scores, k)


def merge_panels(panels, offsets, k):
    """panels: score arrays (nq, ncols_p), the p-th with column offset offsets[p] -> the ranking of their concatenation: what the
    running-list merge of pvs_topk_dev must leave after the last panel, in whatever order the panels arrive"""
    panels = [_float(p) for p in panels]
    nq = panels[0].shape[0]
    vals = np.concatenate(panels, axis=1)
    ids = np.concatenate([np.arange(p.shape[1], dtype=np.int64) + int(o) for p, o in zip(panels, offsets)])
    return _rows(np.broadcast_to(ids, (nq, len(ids))), vals, k)


def merge_lists(idx_lists, val_lists, k):
    """list mode (pvs_topk_merge_dev): idx_lists int64 / val_lists (n_lists, nq, len) -> the best k of each query's entries; entries
    with id < 0 are skipped, ids are distinct within a query"""
    idx_lists, val_lists = np.asarray(idx_lists, np.int64), _float(val_lists)
    n_lists, nq, ln = val_lists.shape
    return _rows(idx_lists.transpose(1, 0, 2).reshape(nq, n_lists * ln), val_lists.transpose(1, 0, 2).reshape(nq, n_lists * ln), k)


def candidates(ids, vals, k):
    """one candidate row per query, longer than k (the probed scan): ids (nq, len), vals (nq, len); id < 0 is skipped"""
    return _rows(np.asarray(ids, np.int64), _float(vals), k)
