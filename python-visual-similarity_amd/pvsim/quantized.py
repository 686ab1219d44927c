"""Int8 resident index: one signed byte per dimension, ranked by the cosine of the code rows.

A `DeviceIndex` keeps 4 L bytes per image and gives exact cosines; a `CompactIndex` keeps m + 4 bytes after a projection and gives a
short list.  An `Int8Index` stands between them: L bytes (padded to a multiple of 64) and one float32 per image, no training, no
projection, and lists that agree with the exact ones almost everywhere.  A row is scaled by its largest magnitude and rounded to
-127 .. 127; the score of two rows is the cosine of their codes, whose dot product is an int32 -- so every kernel, tiling and order
of summation gives the same bits, and tests/sq8_numpy.py restates it with integer sums.  The definitions are in include/pvsim.h."""
from __future__ import annotations

import numpy as np

from ._ffi import SQ8_MAX_L
from .index import DeviceIndex, _PathLedger, _grow_rows, _keep_positions

__all__ = ["Int8Index", "save_int8_arrays", "load_int8_arrays", "padded_length"]

KIND = "int8_index"
_CHUNK_BYTES = 64 << 20          # float32 rows that go through the device at a time when a host matrix is encoded


_RANGE_PATHS = {"auto": 0, "panel": 1, "mask": 2}          # SQ8_RANGE_PATH_* of pvsim/_ffi.py


def _range_path_code(path) -> int:
    if not isinstance(path, str) or path not in _RANGE_PATHS:
        raise ValueError(f"path must be one of {sorted(_RANGE_PATHS)}, got {path!r}")
    return _RANGE_PATHS[path]


def padded_length(L: int) -> int:
    """ld = 64 ceil(L / 64): the bytes of a stored code row (PVS_SQ8_LD of include/pvsim.h)"""
    return 64 * ((int(L) + 63) // 64)


def _all_finite(a: np.ndarray) -> bool:
    """A finite sum of squares (one BLAS pass, no temporary) proves every element finite: a NaN or an infinity survives the
    products and the additions.  The sum of a finite row may overflow, so anything else is looked at element by element."""
    flat = a.reshape(-1)
    return bool(np.isfinite(np.dot(flat, flat))) or bool(np.isfinite(a).all())


def _f32_rows(a, what: str) -> np.ndarray:
    """float32 2-d rows, finite, C-contiguous; float64 is a TypeError as for a CompactIndex"""
    a = np.asarray(a)
    if a.dtype == np.float64:
        raise TypeError(f"{what} is float64: the int8 index is built from float32 rows, pass float32 {what}")
    if a.dtype != np.float32:
        raise TypeError(f"{what} must be float32, got {a.dtype}")
    if a.ndim != 2:
        raise ValueError(f"{what} must be a 2-d array, got shape {a.shape}")
    a = np.ascontiguousarray(a)
    if not _all_finite(a):
        raise ValueError(f"{what} holds a NaN or an infinity: the int8 codes are defined for finite rows only")
    return a


def _check_length(L: int) -> int:
    if not 1 <= L <= SQ8_MAX_L:
        raise ValueError(f"an int8 index takes rows of 1 <= L <= {SQ8_MAX_L} dimensions (127^2 L must stay below 2^31), got L={L}")
    return int(L)


# ------------------------------------------------------------------------------------------------ persistence (no device needed)
def save_int8_arrays(path: str, paths, codes, factors, L: int) -> None:
    """One plain .npz (numpy.load(allow_pickle=False)): kind, paths, codes int8 (N, L) without the padding, factors float32 (N,), L."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    factors = np.ascontiguousarray(factors, dtype=np.float32)
    paths = [str(p) for p in paths]
    if codes.ndim != 2 or codes.shape != (len(paths), int(L)) or factors.shape != (len(paths),):
        raise ValueError(f"codes must be int8 ({len(paths)}, {L}) and factors float32 ({len(paths)},), got {codes.shape} and {factors.shape}")
    np.savez(path, kind=KIND, paths=np.array(paths, dtype=np.str_), codes=codes, factors=factors, L=np.int64(L))


def load_int8_arrays(path: str) -> dict:
    """-> dict(paths, codes int8 (N, L), factors float32 (N,), L); a file of another kind is a ValueError"""
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
        if "kind" not in z.files or str(z["kind"]) != KIND:
            raise ValueError(f"{path}: not an int8 index file")
        out = dict(paths=[str(p) for p in z["paths"]], codes=z["codes"], factors=z["factors"], L=int(z["L"]))
    n, L = len(out["paths"]), out["L"]
    if out["codes"].dtype != np.int8 or out["codes"].shape != (n, L) or out["factors"].dtype != np.float32 or out["factors"].shape != (n,):
        raise ValueError(f"{path}: the arrays of the int8 index file do not fit each other")
    return out


# ------------------------------------------------------------------------------------------------ index
class Int8Index:
    """Paths + int8 codes (N, ld) + float32 row factors (N,) resident on the device, ranked by pvs_sq8_topk_dev.

    `Int8Index(encoding_map)` quantises the float32 vectors of {path: vector}; `Int8Index.from_index(device_index)` reads the
    resident rows of a float32 DeviceIndex in place and leaves it as it is.  Only codes and factors are kept.  `add`, `remove` /
    `del index[path]` and `reserve` change the index without a rebuild: the rule is per row, so nothing is
    retrained, and after any sequence of updates codes and factors equal, byte for byte, those of an index built from the
    surviving rows in surviving order."""

    def __init__(self, encoding_map, ctx=None):
        from .engine import default_context
        paths = [str(p) for p in encoding_map.keys()]
        mat = np.array(list(encoding_map.values()))
        if mat.ndim != 2:
            raise ValueError("Int8Index needs one vector of the same length per entry")
        mat = _f32_rows(mat, "database")
        L = _check_length(mat.shape[1])
        self._init_empty(paths, L, ctx or default_context(), len(paths))
        self._encode_host(mat, 0)

    @classmethod
    def from_index(cls, device_index, ctx=None) -> "Int8Index":
        """The int8 copy of a float32 DeviceIndex: its resident rows are encoded where they lie."""
        if not isinstance(device_index, DeviceIndex):
            raise TypeError("from_index takes a pvsim.index.DeviceIndex")
        if device_index.dtype != np.float32:
            raise TypeError("the DeviceIndex is float64: the int8 index is built from float32 rows")
        n, L = device_index.shape
        L = _check_length(L)
        if not _all_finite(device_index.matrix):
            raise ValueError("database holds a NaN or an infinity: the int8 codes are defined for finite rows only")
        self = cls.__new__(cls)
        self._init_empty(list(device_index.keys()), L, ctx or device_index.ctx, n)
        if n:
            self.ctx.sq8_encode_dev(device_index._db.ptr, n, L, self._codes.ptr, self._inv.ptr)
            self.ctx.sync()
        return self

    @classmethod
    def _from_arrays(cls, paths, codes, factors, L, ctx=None) -> "Int8Index":
        """An index over given codes (N, L) and factors: they go up as they are, nothing is quantised again"""
        from .engine import default_context
        self = cls.__new__(cls)
        n = len(paths)
        self._init_empty(paths, _check_length(L), ctx or default_context(), n)
        if n:
            padded = np.zeros((n, self._ld), np.int8)
            padded[:, :L] = codes
            self._codes.upload(padded)
            self._inv.upload(np.ascontiguousarray(factors, dtype=np.float32))
        return self

    def _init_empty(self, paths, L, ctx, cap):
        self.ctx, self._L, self._ld = ctx, int(L), padded_length(L)
        self._ledger = _PathLedger(paths)
        if len(set(self._ledger.paths)) != len(self._ledger.paths):
            raise ValueError("a path is named twice")
        self._cap = int(cap)
        self.modifications = 0            # adds and removes since construction: a pvsim.Subset is a snapshot of the rows
        self.last_range_stats = None      # what the last threshold search reported
        self._codes = ctx.buffer(max(self._cap * self._ld, 16))
        self._inv = ctx.buffer(max(self._cap * 4, 16))

    def _encode_host(self, mat: np.ndarray, first: int) -> None:
        """host rows -> codes and factors of rows first, first + 1, ...: uploaded a chunk at a time into a scratch scope"""
        L, ld = self._L, self._ld
        step = max(1, _CHUNK_BYTES // (4 * L))
        for r0 in range(0, mat.shape[0], step):
            rn = min(step, mat.shape[0] - r0)
            with self.ctx.scratch() as tmp:
                d_x = tmp.upload(mat[r0:r0 + rn])
                self.ctx.sq8_encode_dev(d_x.ptr, rn, L, self._codes.ptr + (first + r0) * ld, self._inv.ptr + (first + r0) * 4)
                self.ctx.sync()

    # ---- the dict-like surface the retrieval functions use
    @property
    def context(self):
        return self.ctx

    def __len__(self):
        return len(self._ledger)

    def __contains__(self, path):
        return path in self._ledger

    @property
    def paths(self) -> list:
        return list(self._ledger.paths)

    def keys(self):
        return list(self._ledger.paths)

    @property
    def shape(self):
        """(N, L): L is the length of the vectors `rank` takes, not the padded row"""
        return len(self._ledger), self._L

    @property
    def capacity(self) -> int:
        return self._cap

    @property
    def nbytes_breakdown(self) -> dict:
        n = len(self)
        return {"codes": n * self._ld, "factors": n * 4}

    @property
    def nbytes(self) -> int:
        """device bytes of the N rows: N (64 ceil(L / 64) + 4)"""
        return int(sum(self.nbytes_breakdown.values()))

    def _download(self):
        """-> (codes int8 (N, ld) with the padding, factors float32 (N,))"""
        n = len(self)
        if n == 0:
            return np.zeros((0, self._ld), np.int8), np.zeros(0, np.float32)
        return self._codes.download((n, self._ld), np.int8), self._inv.download((n,), np.float32)

    # ---- updates
    def reserve(self, n: int) -> None:
        """Room for n rows in the code and factor buffers (no-op when they already hold that many)."""
        n = int(n)
        if n <= self._cap:
            return
        used = len(self)
        self._codes = _grow_rows(self.ctx, self._codes, self._ld, used, n)
        self._inv = _grow_rows(self.ctx, self._inv, 4, used, n)
        self._cap = n

    def add(self, source) -> None:
        """Append new images: `source` is {path: float32 vector of L} or a float32 DeviceIndex whose resident rows are read in place.
        They get the indices N, N + 1, ... in the order given.  A path that is already indexed is a ValueError, raised before
        anything changes."""
        resident = source if isinstance(source, DeviceIndex) else None
        paths = [str(p) for p in source.keys()]
        if not paths:
            return
        self._ledger.check_new(paths)
        if resident is not None:
            if resident.dtype != np.float32:
                raise TypeError("an int8 index takes float32 vectors, the DeviceIndex is float64")
            mat = resident.matrix
        else:
            mat = np.array(list(source.values()))
        if mat.ndim != 2 or mat.shape[1] != self._L:
            raise ValueError(f"new vectors must have the index's length {self._L}, got an array of shape {mat.shape}")
        mat = _f32_rows(mat, "new vectors")
        n, b = len(self), len(paths)
        if n + b > self._cap:
            self.reserve(max(n + b, 2 * self._cap))
        if resident is not None:
            self.ctx.sq8_encode_dev(resident._db.ptr, b, self._L, self._codes.ptr + n * self._ld, self._inv.ptr + n * 4)
            self.ctx.sync()
        else:
            self._encode_host(mat, n)
        self._ledger.append(paths)
        self.modifications += 1

    def remove(self, paths) -> None:
        """The named images leave, the others keep their order.  An unknown path is a KeyError, a path named twice a ValueError, both
        raised before anything changes.  Codes and factors are compacted in place on the device."""
        idx = self._ledger.removed_indices([paths] if isinstance(paths, str) else [str(p) for p in paths])
        if idx.size == 0:
            return
        n = len(self)
        with self.ctx.scratch() as tmp:
            keep, pos = _keep_positions(tmp, idx, n)
            self.ctx.compact_rows_dev(self._codes.ptr, n, self._ld, keep.ptr, pos.ptr, self._codes.ptr, first=int(idx[0]))
            self.ctx.compact_rows_dev(self._inv.ptr, n, 4, keep.ptr, pos.ptr, self._inv.ptr, first=int(idx[0]))
            self.ctx.sync()
        self._ledger.remove(idx)
        self.modifications += 1

    def __delitem__(self, path) -> None:
        self.remove([path])

    # ---- search
    def subset(self, allowed):
        """A pvsim.Subset of this index: `allowed` is a 1-d integer array of indices in any order, a boolean mask of length N, or an
        iterable of paths.  A snapshot: it refuses once rows were added or removed."""
        from .subset import Subset
        return Subset(self, allowed)

    def rank(self, query_vecs, k: int, allowed=None, subset_path: str = "auto"):
        """-> (idx (nq, k) int64, val (nq, k) float32): the queries are quantised by the rule of the rows and ranked by the cosine of
        the codes, (score descending, index ascending); 1 <= k <= N.
        `allowed` (a pvsim.Subset of this index, or what `subset` takes): the same ranking with every row outside the set deleted,
        1 <= k <= |S| and k <= 1024; `subset_path` "auto", "mask" or "listed" pins how it is computed, never what."""
        if allowed is not None:
            from .subset import rank_subset
            return rank_subset(self, query_vecs, k, allowed, subset_path)
        q = _f32_rows(query_vecs, "query")
        n, L = self.shape
        if q.shape[1] != L:
            raise ValueError(f"query and database dimensions differ: {q.shape[1]} vs {L}")
        if isinstance(k, bool) or int(k) != k or not 1 <= k <= n:
            raise ValueError(f"k must be an integer with 1 <= k <= {n} (the number of indexed rows), got {k!r}")
        k, nq, ctx = int(k), q.shape[0], self.ctx
        if nq == 0:
            return np.zeros((0, k), np.int64), np.zeros((0, k), np.float32)
        with ctx.scratch() as tmp:
            d_q, d_qc, d_invq = tmp.upload(q), tmp(nq * self._ld), tmp(nq * 4)
            d_idx, d_val = tmp(nq * k * 8), tmp(nq * k * 4)
            ctx.sq8_encode_dev(d_q.ptr, nq, L, d_qc.ptr, d_invq.ptr)
            ctx.sq8_topk_dev(d_qc.ptr, d_invq.ptr, nq, self._codes.ptr, self._inv.ptr, n, L, k, 0, False, d_idx.ptr, d_val.ptr)
            return d_idx.download((nq, k), np.int64), d_val.download((nq, k), np.float32)

    # ---- threshold search: everything at least this similar, on the int8 pipe
    def _range_dev(self, tmp, d_qc: int, d_invq: int, nq: int, threshold, limit, path: str, upper: bool):
        """pvs_sq8_range_dev of nq code rows on the device against the stored rows, the triples left on the device: -> (rows int64,
        cols int64, vals float32: DeviceBuffers of the scratch scope `tmp`, total, stats).  Capacity and the one retry are those of
        DeviceIndex._range_dev: max(4096, 4 nq) entries first (`limit` if smaller), then once at the reported total unless that
        exceeds `limit`."""
        from . import _ffi
        n, L = self.shape
        flags = _ffi.RANGE_UPPER if upper else 0
        cap = max(4096, 4 * nq) if limit is None else min(max(4096, 4 * nq), int(limit))
        for attempt in (0, 1):
            bufs = tmp(max(cap, 1) * 8), tmp(max(cap, 1) * 8), tmp(max(cap, 1) * 4)
            try:
                total, stats = self.ctx.sq8_range_dev(d_qc, d_invq, nq, self._codes.ptr, self._inv.ptr, n, L, threshold, cap, bufs[0].ptr,
                                                      bufs[1].ptr, bufs[2].ptr, flags=flags, path=_range_path_code(path))
                return bufs + (total, dict(stats, retried=bool(attempt), threshold=float(threshold)))
            except _ffi.CapacityError as e:
                total = e.args[1]
                if attempt or (limit is not None and total > int(limit)):
                    raise _ffi.CapacityError(f"{total} results exceed the limit of {cap if limit is None else int(limit)}", total) from None
                cap = total

    def range_search(self, query_vecs, threshold: float, *, max_results=None, path: str = "auto"):
        """Every stored row whose score with a query is at least `threshold` (rounded once to float32; the comparison is in float32
        on the score `rank` reports: the queries are quantised by the rule of the rows) -> CSR (indptr int64 (nq + 1,), indices int64,
        scores float32), per query (score descending, index ascending).  `max_results` bounds the total over all queries: more raises
        CapacityError carrying the total (args[1]).  path: "auto", "panel" (float panels thresholded) or "mask" (one bit per pair from
        the int8 GEMM); the result is the same bytes.  `last_range_stats` holds what the device reported."""
        from .duplicates import _check_limit, _check_threshold
        t = _check_threshold(threshold)
        limit = _check_limit("max_results", max_results)
        _range_path_code(path)
        q = _f32_rows(query_vecs, "query")
        n, L = self.shape
        if q.shape[1] != L:
            raise ValueError(f"query and database dimensions differ: {q.shape[1]} vs {L}")
        nq, ctx = q.shape[0], self.ctx
        if nq == 0 or n == 0:
            self.last_range_stats = {"threshold": float(t)}
            return np.zeros(nq + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        with ctx.scratch() as tmp:
            d_q, d_qc, d_invq = tmp.upload(q), tmp(nq * self._ld), tmp(nq * 4)
            ctx.sq8_encode_dev(d_q.ptr, nq, L, d_qc.ptr, d_invq.ptr)
            d_row, d_col, d_val, total, self.last_range_stats = self._range_dev(tmp, d_qc.ptr, d_invq.ptr, nq, t, limit, path, False)
            row, col, val = (d_row.download((total,), np.int64), d_col.download((total,), np.int64), d_val.download((total,), np.float32))
        order = np.lexsort((col, -val, row))                 # one stable sort; -0 and +0 tie and the index decides
        indptr = np.zeros(nq + 1, np.int64)
        np.cumsum(np.bincount(row, minlength=nq), out=indptr[1:])
        return indptr, col[order], val[order]

    def similar_pairs(self, threshold: float, *, max_pairs=None, path: str = "auto"):
        """The self-join -> (i int64, j int64, score float32) in (i, j) order: every pair of stored rows i < j with s(i, j) >=
        `threshold`, where s(i, j) is the score `rank` of stored row i reports for row j (row i in the query role).  The int8 score
        is two separately rounded products, ((float)acc * inv_i) * inv_j, and is NOT symmetric: a pair with s(i, j) < threshold <=
        s(j, i) is not returned.  `max_pairs` bounds the number of pairs: more raises CapacityError carrying the total."""
        from .duplicates import _check_limit, _check_threshold
        t = _check_threshold(threshold)
        limit = _check_limit("max_pairs", max_pairs)
        _range_path_code(path)
        n = self.shape[0]
        if n == 0:
            self.last_range_stats = {"threshold": float(t)}
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        with self.ctx.scratch() as tmp:
            d_row, d_col, d_val, total, self.last_range_stats = self._range_dev(tmp, self._codes.ptr, self._inv.ptr, n, t, limit, path, True)
            row, col, val = (d_row.download((total,), np.int64), d_col.download((total,), np.int64), d_val.download((total,), np.float32))
        order = np.lexsort((col, row))
        return row[order], col[order], val[order]

    def duplicates(self, threshold: float, *, min_size: int = 2, path: str = "auto"):
        """-> pvsim.DuplicateGroups: the connected components of the pairs of `similar_pairs` (the same definition: s(i, j), i < j, row
        i in the query role).  The join and the components run on the device and the pairs stay there in between."""
        from .duplicates import _check_min_size, _check_threshold, _groups_of_self_join
        t = _check_threshold(threshold)
        _range_path_code(path)

        def join(tmp, n):
            out = self._range_dev(tmp, self._codes.ptr, self._inv.ptr, n, t, None, path, True)
            self.last_range_stats = out[4]
            return out
        return _groups_of_self_join(self, t, _check_min_size(min_size), join)

    # ---- persistence
    def save(self, path: str) -> None:
        codes, inv = self._download()
        save_int8_arrays(path, self._ledger.paths, codes[:, :self._L], inv, self._L)

    @classmethod
    def load(cls, path: str, ctx=None) -> "Int8Index":
        a = load_int8_arrays(path)
        return cls._from_arrays(a["paths"], a["codes"], a["factors"], a["L"], ctx)

    def close(self):
        for b in (self._codes, self._inv):
            b.free()
