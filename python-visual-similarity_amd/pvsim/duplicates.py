"""Near-duplicate search on a resident index: the cosine threshold join and the groups it connects.

Every ranker answers "the k best"; this answers "everything at least this similar".  `DeviceIndex.range_search` returns every row
above a score for each query, `DeviceIndex.similar_pairs` every pair of rows of the index above it, and `find_duplicates` the
connected components of those pairs: the groups of near duplicates a corpus is cleaned of before it is indexed.  The join
(pvs_cosine_range_dev) and the components (pvs_pair_components_dev) run on the device and the pair list stays there between them; the
score is the float32 value every ranking of the index reports, and the result does not depend on the path taken.

An `Int8Index` has the same three answers on its own code rows (pvs_sq8_range_dev) as methods: `range_search`,
`similar_pairs` and `duplicates`.  The free functions here serve the float32 DeviceIndex only and say so."""
from __future__ import annotations

import numpy as np

from . import _ffi

__all__ = ["DuplicateGroups", "find_duplicates"]

_PATHS = {"auto": _ffi.RANGE_PATH_AUTO, "exact": _ffi.RANGE_PATH_EXACT, "filtered": _ffi.RANGE_PATH_FILTERED}


def _path_code(path) -> int:
    if path not in _PATHS:
        raise ValueError(f"path must be one of {sorted(_PATHS)}, got {path!r}")
    return _PATHS[path]


def _check_threshold(threshold) -> np.float32:
    """the user's number rounded ONCE to float32: the value the device compares with, and the one reported back"""
    if isinstance(threshold, (bool, str)) or not np.isscalar(threshold):
        raise TypeError(f"threshold must be a real number, got {threshold!r}")
    with np.errstate(over="ignore"):
        t = np.float32(threshold)
    if not np.isfinite(t):
        raise ValueError(f"threshold must be a finite float32, got {threshold!r}")
    return t


def _check_limit(name: str, value):
    if value is None:
        return None
    if isinstance(value, bool) or int(value) != value or not 0 <= value <= _ffi.RANGE_MAX_CAPACITY:
        raise ValueError(f"{name} must be None or an integer in [0, 2^40], got {value!r}")
    return int(value)


def _check_index(index) -> None:
    """the float32 DeviceIndex only: float64, int8 and compact indexes are named and refused (an Int8Index is pointed to its methods)"""
    from .index import DeviceIndex
    if not isinstance(index, DeviceIndex):
        own = (": an Int8Index has its own range_search, similar_pairs and duplicates methods (DESIGN.md section 30)"
               if type(index).__name__ == "Int8Index" else "")
        raise NotImplementedError(f"threshold search runs on a float32 pvsim.index.DeviceIndex, not on a {type(index).__name__}{own}")
    if index.dtype != np.float32:
        raise NotImplementedError(f"threshold search runs on a float32 pvsim.index.DeviceIndex: this one holds {index.dtype} rows")


class DuplicateGroups:
    """What `find_duplicates` found.  labels int64 (N,): the smallest index of every row's group (its own for a row alone); groups:
    index arrays, members ascending, groups by first member, those of at least `min_size` rows; paths: the same as lists of paths;
    pairs: (i, j, score) of the join, i < j, in (i, j) order; stats: threshold (the float32 value compared with), pairs, components,
    rounds, and what the join reported."""

    def __init__(self, labels, groups, paths, pairs, stats):
        self.labels, self.groups, self.paths, self.pairs, self.stats = labels, groups, paths, pairs, stats

    def __len__(self):
        return len(self.groups)

    def __iter__(self):
        return iter(self.paths)


def find_duplicates(index, threshold: float, *, min_size: int = 2, path: str = "auto") -> DuplicateGroups:
    """Groups of rows connected by pairs whose cosine is at least `threshold`: the join and the components run on the device and the
    pairs stay there in between; labels and pairs come down once."""
    _check_index(index)
    t = _check_threshold(threshold)
    _path_code(path)
    return _groups_of_self_join(index, t, _check_min_size(min_size),
                                lambda tmp, n: index._range_dev(tmp, index._db.ptr, n, index._inv.ptr, t, None, path, True))


def _check_min_size(min_size) -> int:
    if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 1:
        raise ValueError(f"min_size must be a positive integer, got {min_size!r}")
    return int(min_size)


def _groups_of_self_join(index, t, min_size: int, join) -> DuplicateGroups:
    """`join(tmp, n)` -> (rows, cols, vals on the device, total, stats): the self-join of the index's n rows, left in the scratch
    scope `tmp`; the components are labelled on those pairs where they lie, labels and pairs come down once."""
    n = index.shape[0]
    if n == 0:
        empty = np.zeros(0, np.int64)
        return DuplicateGroups(empty, [], [], (empty, empty.copy(), np.zeros(0, np.float32)),
                               {"threshold": float(t), "pairs": 0, "components": 0, "rounds": 0})
    with index.ctx.scratch() as tmp:
        d_row, d_col, d_val, total, stats = join(tmp, n)
        d_label = tmp(n * 4)
        comp = index.ctx.pair_components_dev(d_row.ptr, d_col.ptr, total, n, d_label.ptr)
        labels = d_label.download((n,), np.int32).astype(np.int64)
        row, col, val = (d_row.download((total,), np.int64), d_col.download((total,), np.int64), d_val.download((total,), np.float32))
    order = np.lexsort((col, row))
    members = np.argsort(labels, kind="stable")                      # by label = first member, members ascending within one
    cuts = np.flatnonzero(np.diff(labels[members])) + 1
    groups = [g for g in np.split(members, cuts) if g.size >= int(min_size)]
    names = index._ledger.paths
    return DuplicateGroups(labels, groups, [[names[i] for i in g] for g in groups], (row[order], col[order], val[order]),
                           dict(stats, pairs=int(total), **comp))
