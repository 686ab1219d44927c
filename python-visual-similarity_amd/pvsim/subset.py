"""Subset search: the k best among an allowed set of images.

`index.subset(allowed)` turns "these images" -- indices, a boolean mask or paths -- into a `Subset` of a float32 `DeviceIndex` or an
`Int8Index`; `index.rank(q, k, allowed=...)` then returns the index's full ranking with every row outside the set deleted, cut to k:
the same order, the same indices and the same score bits as `rank(q, N)` filtered on the host, whatever the path.  A `Subset` is a
snapshot of the index it was made for and refuses to rank once rows were added or removed."""
from __future__ import annotations

import numpy as np

from . import _ffi

__all__ = ["Subset", "normalise"]

_PATHS = {"auto": _ffi.SUBSET_PATH_AUTO, "mask": _ffi.SUBSET_PATH_MASK, "listed": _ffi.SUBSET_PATH_LISTED}


def _path_code(path) -> int:
    if path not in _PATHS:
        raise ValueError(f"subset_path must be 'auto', 'mask' or 'listed', got {path!r}")
    return _PATHS[path]


def normalise(allowed, n: int, index_of=None) -> np.ndarray:
    """`allowed` -> sorted int64 ids within [0, n).  One of: a boolean mask of length n; a 1-d integer array in any order (a duplicate
    is a ValueError, an index outside [0, n) an IndexError); an iterable of paths, resolved by `index_of(path)` (KeyError for an unknown
    path, ValueError for one named twice).  An empty set is a ValueError."""
    n = int(n)
    if isinstance(allowed, (str, bytes)):
        allowed = [allowed]
    arr = allowed if isinstance(allowed, np.ndarray) else np.array(list(allowed))
    if arr.dtype == np.bool_:
        if arr.ndim != 1 or arr.shape[0] != n:
            raise ValueError(f"a boolean mask must have one entry per indexed row: shape ({n},), got {arr.shape}")
        ids = np.flatnonzero(arr).astype(np.int64)
    elif arr.size == 0:
        ids = np.zeros(0, np.int64)
    elif arr.dtype.kind in "iu":
        if arr.ndim != 1:
            raise ValueError(f"allowed indices must be a 1-d array, got shape {arr.shape}")
        if int(arr.min()) < 0 or int(arr.max()) >= n:
            bad = arr[(arr < 0) | (arr >= n)][0]
            raise IndexError(f"allowed index {int(bad)} is outside [0, {n})")
        ids = np.sort(arr.astype(np.int64))
        if ids.size > 1 and bool((ids[1:] == ids[:-1]).any()):
            raise ValueError(f"allowed index {int(ids[1:][ids[1:] == ids[:-1]][0])} is named twice")
    elif arr.dtype.kind in "USO":
        if index_of is None:
            raise TypeError("paths need an index that knows them")
        seen, found = set(), []
        for p in arr.reshape(-1).tolist():
            try:
                i = int(index_of(p))
            except (KeyError, ValueError):
                raise KeyError(p) from None
            if i in seen:
                raise ValueError(f"{p!r} is named twice in the allowed set")
            seen.add(i)
            found.append(i)
        ids = np.sort(np.array(found, dtype=np.int64))
    else:
        raise TypeError(f"allowed must be integer indices, a boolean mask or paths, got an array of {arr.dtype}")
    if ids.size == 0:
        raise ValueError("the allowed set is empty: a subset ranking needs at least one row")
    return ids


def _kind(index) -> str:
    from .index import DeviceIndex
    from .quantized import Int8Index
    if isinstance(index, Int8Index):
        return "int8"
    if isinstance(index, DeviceIndex):
        if index.dtype != np.float32:
            raise TypeError("subset search is built for a float32 DeviceIndex and an Int8Index: this DeviceIndex is float64 "
                            "(its split-K plan makes a score depend on the panel)")
        return "f32"
    raise ValueError(f"subset search is built for a float32 DeviceIndex and an Int8Index, not for {type(index).__name__}")


def _index_of(index):
    ledger = index._ledger

    def index_of(path):
        if path not in ledger:
            raise KeyError(path)
        return ledger.index_of(path)
    return index_of


class Subset:
    """An allowed set of rows of ONE index, on the device: sorted ids and a bitmask of the index's rows (pvs_subset_create).
    `ids` is the host copy, `len(subset)` the size.  A snapshot: after `add`, `remove` or `del` on the index, ranking with it raises a
    ValueError (the ids would name other rows); make a new one.  `close()`, or garbage collection, frees the device arrays."""

    def __init__(self, index, allowed):
        self.kind = _kind(index)
        self.index, self.n = index, len(index)
        if self.n == 0:
            raise ValueError("the index is empty: there is no row to allow")
        self.ids = normalise(allowed, self.n, _index_of(index))
        self.ids.setflags(write=False)
        self._mods = index.modifications
        self._handle = index.ctx.subset_create(self.ids, self.n)

    def __len__(self):
        return int(self.ids.size)

    @property
    def handle(self):
        return self._handle

    def check(self, index) -> None:
        """ValueError unless this subset can rank on `index` now"""
        if self._handle is None or self._handle.handle is None:
            raise ValueError("this Subset is closed")
        if index is not self.index:
            raise ValueError("this Subset was made for another index: make one with index.subset(allowed)")
        if index.modifications != self._mods or len(index) != self.n:
            raise ValueError("the index has changed since this Subset was made (rows were added or removed): make a new one with "
                             "index.subset(allowed)")

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_k(k, size: int) -> int:
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= size:
        raise ValueError(f"k must be an integer with 1 <= k <= {size} (the size of the allowed set), got {k!r}")
    if k > _ffi.SUBSET_MAX_K:
        raise ValueError(f"a subset ranking holds at most {_ffi.SUBSET_MAX_K} entries, got k = {k}: deeper lists are not built")
    return int(k)


def rank_subset(index, query_vecs, k, allowed, subset_path: str = "auto", tile: int = 0):
    """`index.rank(query_vecs, k, allowed=allowed, subset_path=subset_path)`; `tile` > 0 cuts the panels and chunks (tests).
    `allowed`: a Subset of this index, or anything `index.subset` takes (a temporary Subset is made and destroyed here).
    -> (idx (nq, k) int64 in the numbering of the full index, val (nq, k) float32); index.last_subset_stats holds the device's report."""
    kind = _kind(index)
    code = _path_code(subset_path)
    q = np.asarray(query_vecs)
    L = index.shape[1]
    if kind == "f32":
        if q.ndim != 2 or q.shape[1] != L:
            raise ValueError("query and database dimensions differ")
        if q.dtype != np.float32:
            raise TypeError(f"subset search scores in float32: float32 queries on a float32 DeviceIndex, got {q.dtype}")
        q = np.ascontiguousarray(q)
    else:
        from .quantized import _f32_rows
        q = _f32_rows(q, "query")
        if q.shape[1] != L:
            raise ValueError(f"query and database dimensions differ: {q.shape[1]} vs {L}")
    temp = None if isinstance(allowed, Subset) else Subset(index, allowed)
    sub = temp or allowed
    try:
        sub.check(index)
        k = _check_k(k, len(sub))
        nq, n, ctx = q.shape[0], sub.n, index.ctx
        if nq == 0:
            index.last_subset_stats = None
            return np.zeros((0, k), np.int64), np.zeros((0, k), np.float32)
        with ctx.scratch() as tmp:
            d_q, d_invq = tmp.upload(q), tmp(nq * 4)
            d_idx, d_val = tmp(nq * k * 8), tmp(nq * k * 4)
            if kind == "f32":
                index._row_inv_norms(d_q.ptr, nq, d_invq.ptr)
                index.last_subset_stats = ctx.cosine_topk_subset_dev(d_q.ptr, nq, index._db.ptr, n, L, d_invq.ptr, index._inv.ptr, sub.handle,
                                                                     k, d_idx.ptr, d_val.ptr, path=code, tile=tile)
            else:
                d_qc = tmp(nq * index._ld)
                ctx.sq8_encode_dev(d_q.ptr, nq, L, d_qc.ptr, d_invq.ptr)
                index.last_subset_stats = ctx.sq8_topk_subset_dev(d_qc.ptr, d_invq.ptr, nq, index._codes.ptr, index._inv.ptr, n, L, sub.handle,
                                                                  k, d_idx.ptr, d_val.ptr, path=code, tile=tile)
            return d_idx.download((nq, k), np.int64), d_val.download((nq, k), np.float32)
    finally:
        if temp is not None:
            temp.close()
