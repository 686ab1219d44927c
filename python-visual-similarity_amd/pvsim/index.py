"""Encoding-map persistence: the reference keeps its index as an in-memory dict {image_path: vector}
(`generate_encoding_map`, pyvisim/encoders/_base_encoder.py:344-359) and only offers generic HDF5 helpers.
Here an index is one plain `.npz` per shard (paths + one (n, L) matrix): no pickles, loadable with
numpy.load(allow_pickle=False), and shaped for the sharded multi-GPU layout (one file per rank)."""
from __future__ import annotations

import os
from collections.abc import Mapping

import numpy as np

__all__ = ["save_encoding_map", "load_encoding_map", "save_shard", "load_shards", "DeviceIndex"]


def save_encoding_map(path: str, encoding_map: dict) -> None:
    """{path: (L,) vector} -> <path>.npz, preserving insertion order (= database index order, eval.py:28)."""
    keys = list(encoding_map.keys())
    mat = np.vstack([np.asarray(encoding_map[k]).reshape(1, -1) for k in keys]) if keys else np.zeros((0, 0), np.float32)
    np.savez(path, paths=np.array(keys, dtype=np.str_), vectors=mat)


def load_encoding_map(path: str) -> dict:
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
        return dict(zip([str(p) for p in z["paths"]], z["vectors"]))


def save_shard(directory: str, rank: int, world: int, first_index: int, vectors: np.ndarray, paths=None) -> str:
    """One rank's contiguous block of the corpus (images [first_index, first_index + n))."""
    os.makedirs(directory, exist_ok=True)
    fn = os.path.join(directory, f"shard_{rank:04d}_of_{world:04d}.npz")
    np.savez(fn, first_index=np.int64(first_index), vectors=np.ascontiguousarray(vectors),
             paths=np.array(list(paths) if paths is not None else [], dtype=np.str_))
    return fn


def load_shards(directory: str):
    """-> (vectors (N, L) in global index order, paths list) from every shard file of `directory`."""
    files = sorted(f for f in os.listdir(directory) if f.startswith("shard_") and f.endswith(".npz"))
    parts = []
    for f in files:
        with np.load(os.path.join(directory, f), allow_pickle=False) as z:
            parts.append((int(z["first_index"]), z["vectors"], [str(p) for p in z["paths"]]))
    parts.sort(key=lambda p: p[0])
    vecs = np.vstack([p[1] for p in parts]) if parts else np.zeros((0, 0), np.float32)
    return vecs, [q for p in parts for q in p[2]]


def _removed_indices(paths, pos: dict) -> np.ndarray:
    """paths to remove -> their indices, ascending int64; KeyError for an unknown path, ValueError for one named twice"""
    paths = [paths] if isinstance(paths, str) else list(paths)
    seen = set()
    for p in paths:
        if p not in pos:
            raise KeyError(p)
        if p in seen:
            raise ValueError(f"{p!r} is named twice in one remove")
        seen.add(p)
    return np.sort(np.array([pos[p] for p in paths], dtype=np.int64))


def _keep_positions(tmp, idx: np.ndarray, n: int):
    """ascending removed indices -> (keep mask uint8 (n,), positions int64 (n + 1,)) as device buffers of the scratch scope `tmp`
    (Context.scratch): idx.size indices go up"""
    d_idx, keep, pos = tmp.upload(idx), tmp(n), tmp((n + 1) * 8)
    tmp.ctx.keep_mask_dev(d_idx.ptr, idx.size, n, keep.ptr)
    tmp.ctx.keep_positions_dev(keep.ptr, n, pos.ptr)
    return keep, pos


def _grow_rows(ctx, buf, row_bytes: int, used: int, need: int):
    """-> a device buffer of `need` rows that holds the first `used` rows of `buf` (copied on the device); `buf` is freed"""
    new = ctx.buffer(need * row_bytes)
    if used * row_bytes:
        ctx.copy_dev(new.ptr, buf.ptr, used * row_bytes)
    buf.free()
    return new


def _compact_host_rows(buf: np.ndarray, n: int, idx: np.ndarray) -> None:
    """rows idx (ascending) leave the first n rows of buf, in place: one block move per run of kept rows"""
    dst = int(idx[0])
    bounds = np.append(idx, n)
    for j in range(idx.size):
        a, b = int(bounds[j]) + 1, int(bounds[j + 1])
        if b > a:
            buf[dst:dst + b - a] = buf[a:b]
            dst += b - a


def _compact_list(items: list, idx: np.ndarray) -> list:
    """the list without the entries at idx (ascending): one slice per run of kept entries"""
    out, prev = [], 0
    for i in idx.tolist():
        out.extend(items[prev:i])
        prev = i + 1
    out.extend(items[prev:])
    return out


class _PathLedger:
    """Which path stands at which position of a mutable index, across adds and removes.

    A path gets a serial number when it joins; serials rise with the position, so the position of a path is the rank of its serial
    among the live ones (`_live`, ascending int64).  A remove deletes entries and renumbers nothing: the interpreter's share of an
    update is O(b) for an add and O(r) for a remove, beside one array copy and the list slices.  `paths` is the list in index order."""

    def __init__(self, paths=()):
        self.paths = list(paths)
        self._next = len(self.paths)
        self._serial = {p: i for i, p in enumerate(self.paths)}
        self._live = np.arange(self._next, dtype=np.int64)

    def __len__(self):
        return len(self.paths)

    def __contains__(self, path):
        return path in self._serial

    def index_of(self, path) -> int:
        return int(np.searchsorted(self._live, self._serial[path]))

    def check_new(self, paths) -> None:
        """ValueError for a path that is already indexed or named twice in `paths`; nothing changes"""
        seen = set()
        for p in paths:
            if p in self._serial:
                raise ValueError(f"{p!r} is already indexed: remove it first")
            if p in seen:
                raise ValueError(f"{p!r} is named twice in one add")
            seen.add(p)

    def removed_indices(self, paths) -> np.ndarray:
        """paths to remove -> their positions, ascending int64 (KeyError / ValueError as _removed_indices); nothing changes"""
        return np.searchsorted(self._live, _removed_indices(paths, self._serial))

    def append(self, paths) -> None:
        for i, p in enumerate(paths, self._next):
            self._serial[p] = i
        self._live = np.concatenate([self._live, np.arange(self._next, self._next + len(paths), dtype=np.int64)])
        self._next += len(paths)
        self.paths.extend(paths)

    def remove(self, idx: np.ndarray) -> None:
        """the entries at positions idx (ascending, as removed_indices gives them) leave"""
        for i in idx.tolist():
            del self._serial[self.paths[i]]
        self.paths = _compact_list(self.paths, idx)
        self._live = np.delete(self._live, idx)


class DeviceIndex(Mapping):
    """An encoding map {image_path: vector} whose vectors ALSO live on the GPU, uploaded and normalised once.

    The reference's retrieval functions take the index as a dict and rebuild the (N, L) matrix from it on every call
    (`np.array(list(dataset.values()))`, pyvisim/eval.py:28,65,121) -- for one query image against a resident database that copy
    and its upload are the whole cost.  A DeviceIndex is a read-only Mapping with the dict's keys, order and rows, so it can be
    passed wherever `eval.retrieve_top_k_similar` / `top_k_map` / `top_k_accuracy` take `dataset` / `encoding_map`; they then
    rank against the resident copy (pvs_cosine_topk_dev / pvs_cosine_topk_filtered_dev / pvs_cosine_topk_f64_dev: the same lists
    and scores, bit for bit, as with the dict).  dtype rule of the reference (pyvisim/_utils.py:312-330): float32 scores iff the
    database AND the queries are float32, float64 otherwise.
    `rank_expanded` re-queries with the first results folded into the query, and `augmented` builds the index whose rows have their
    neighbours folded in (pvsim/expand.py); both sum whole rows on the device.
    `add`, `remove` / `del index[path]` and `reserve` change the resident index without a rebuild: rows move
    on the device, and after any sequence of them every array and every ranking equals those of DeviceIndex(dict of the surviving
    rows in surviving order), bit for bit.  `modifications` counts them: a pvsim.Diffusion graph is a snapshot of the rows it was built
    from and refuses to rank once the count has moved.  A mutable graph (`Diffusion.build(index, mutable=True)`)
    is updated THROUGH the graph: `g.add` / `g.remove` change this index and bring the graph along; an `add` or `remove` called here
    directly makes a mutable graph as stale as any other."""

    def __init__(self, encoding_map, ctx=None):
        from .engine import default_context
        self.ctx = ctx or default_context()
        self._paths = encoding_map.keys()
        mat = np.array(list(encoding_map.values()))                      # as the reference builds it (eval.py:28)
        if mat.ndim != 2:
            raise ValueError("DeviceIndex needs one vector of the same length per entry")
        self._hbuf = np.ascontiguousarray(mat, dtype=np.float32 if mat.dtype == np.float32 else np.float64)
        n, L = self._hbuf.shape
        self._db = self.ctx.buffer(self._hbuf.nbytes)
        if n and L:
            self._db.upload(self._hbuf)
        self._finish()

    @classmethod
    def _from_device(cls, paths, d_rows, n, L, dtype, ctx) -> "DeviceIndex":
        """An index over rows that are already on the device (`d_rows`, a DeviceBuffer the index takes over): downloads the host copy
        the Mapping serves and computes the norms with the kernel every index uses."""
        self = cls.__new__(cls)
        self.ctx, self._paths, self._db = ctx, paths, d_rows
        self._hbuf = d_rows.download((n, L), dtype) if n and L else np.zeros((n, L), dtype)
        self._finish()
        return self

    @property
    def _paths(self) -> list:
        """the paths in index order: the ledger's own list, not a copy"""
        return self._ledger.paths

    @_paths.setter
    def _paths(self, paths):
        self._ledger = _PathLedger(paths)

    @property
    def shape(self):
        """(N, L), read without touching the host mirror"""
        return len(self._ledger), self._hbuf.shape[1]

    @property
    def dtype(self):
        """float32 or float64: the dtype of the rows, of the norms and of a ranking's scores"""
        return self._hbuf.dtype

    @property
    def _host(self) -> np.ndarray:
        """The first N rows of the host mirror.  A remove leaves the mirror as it was and notes what left (moving a gigabyte of host
        rows would cost a hundred times what the device's compaction costs); adds behind it are noted too.  The notes are applied
        here, in order, when someone asks for host rows."""
        if self._pending:
            n = self._mirror_rows
            for op, arg in self._pending:
                if op == "remove":
                    _compact_host_rows(self._hbuf, n, arg)
                    n -= arg.size
                else:
                    self._grow_mirror(n, n + arg.shape[0])
                    self._hbuf[n:n + arg.shape[0]] = arg
                    n += arg.shape[0]
            self._pending, self._mirror_rows = [], n
        return self._hbuf[:self._mirror_rows]

    def _grow_mirror(self, used: int, need: int) -> None:
        if need > self._hbuf.shape[0]:
            grown = np.empty((max(need, self._cap), self._hbuf.shape[1]), self._hbuf.dtype)
            grown[:used] = self._hbuf[:used]
            self._hbuf = grown

    def _finish(self):
        n, L = self.shape
        self._pending, self._mirror_rows, self._cap = [], n, n      # host-mirror notes, rows the mirror holds, rows the device buffers hold
        self.modifications = 0                                      # adds and removes since construction
        self._inv = self.ctx.buffer(n * self._hbuf.itemsize)
        self._inv_host = None
        if n and L:
            self._row_inv_norms(self._db.ptr, n, self._inv.ptr)

    def _row_inv_norms(self, d_rows: int, rows: int, d_inv: int) -> None:
        """1 / ||row|| of device rows of the index's dtype and length, by the kernel every ranking uses"""
        (self.ctx.row_inv_norms_dev if self.dtype == np.float32 else self.ctx.row_inv_norms_f64_dev)(d_rows, rows, self.shape[1], d_inv)

    # ---- Mapping: the dict's view of the same rows
    def __getitem__(self, path):
        return self._host[self._ledger.index_of(path)]

    def __iter__(self):
        return iter(self._paths)

    def __len__(self):
        return len(self._ledger)

    @property
    def matrix(self) -> np.ndarray:
        """(N, L) host copy in index order (= np.array(list(d.values())))."""
        return self._host

    @property
    def inv_norms(self) -> np.ndarray:
        """(N,) host copy of the device's 1 / ||row||, in the index's dtype (downloaded once)."""
        if self._inv_host is None:
            n, L = self.shape
            self._inv_host = self._inv.download((n,), self._hbuf.dtype) if n and L else np.zeros(n, self._hbuf.dtype)
        return self._inv_host

    # ---- updates
    @property
    def capacity(self) -> int:
        """rows the device buffers hold without growing (the host mirror follows when it is next written)"""
        return self._cap

    def reserve(self, n: int) -> None:
        """Room for n rows in the device row buffer and the norms, and in the host mirror (no-op when they already hold that many)."""
        n = int(n)
        used, L = self.shape
        if n <= self._cap:
            return
        isz = self._hbuf.dtype.itemsize
        self._db = _grow_rows(self.ctx, self._db, L * isz, used, n)
        self._inv = _grow_rows(self.ctx, self._inv, isz, used, n)
        self._cap = n
        if not self._pending:
            self._grow_mirror(used, n)

    def add(self, encoding_map) -> None:
        """Append the entries of {path: vector} in their order: they get the indices N, N + 1, ....  A path that is already indexed is
        a ValueError, raised before anything changes (there is no in-place replace: remove first).  The rows go up once, and their
        norms come from the kernel every index uses."""
        paths = list(encoding_map.keys())
        if not paths:
            return
        self._ledger.check_new(paths)
        n, L = self.shape
        dt = self._hbuf.dtype
        new = np.array(list(encoding_map.values()))
        if new.ndim != 2 or new.shape[1] != L:
            raise ValueError(f"new vectors must have the index's length {L}, got an array of shape {new.shape}")
        if dt == np.float32 and new.dtype != np.float32:
            raise TypeError(f"a float32 index takes float32 vectors, got {new.dtype}")
        new = np.ascontiguousarray(new, dtype=dt)
        b = new.shape[0]
        if n + b > self._cap:
            self.reserve(max(n + b, 2 * self._cap))
        if self._pending:                                           # the mirror is behind: this add joins the notes
            self._pending.append(("add", new))
        else:
            self._grow_mirror(n, n + b)
            self._hbuf[n:n + b] = new
            self._mirror_rows = n + b
        if L:
            isz = dt.itemsize
            self._db.upload(new, offset=n * L * isz)
            self._row_inv_norms(self._db.ptr + n * L * isz, b, self._inv.ptr + n * isz)
        self._ledger.append(paths)
        self._inv_host = None
        self.modifications += 1

    def remove(self, paths) -> None:
        """The named entries leave; the others keep their order, as `del d[k]` on the dict does.  An unknown path is a KeyError, a
        path named twice a ValueError, both raised before anything changes.  Rows and norms are compacted in place on the device."""
        idx = self._ledger.removed_indices(paths)
        if idx.size == 0:
            return
        n, L = self.shape
        isz = self._hbuf.dtype.itemsize
        if L:
            with self.ctx.scratch() as tmp:
                keep, pos = _keep_positions(tmp, idx, n)
                self.ctx.compact_rows_dev(self._db.ptr, n, L * isz, keep.ptr, pos.ptr, self._db.ptr, first=int(idx[0]))
                self.ctx.compact_rows_dev(self._inv.ptr, n, isz, keep.ptr, pos.ptr, self._inv.ptr, first=int(idx[0]))
        self._pending.append(("remove", idx))
        self._ledger.remove(idx)
        self._inv_host = None
        self.modifications += 1

    def __delitem__(self, path) -> None:
        self.remove([path])

    def _rank_dev_buffers(self, tmp, d_q: int, nq: int, k: int):
        """the ranking behind `_rank_dev` with the lists left on the device -> (1 / ||q|| (nq,), idx int64 (nq, k), val (nq, k)), three
        DeviceBuffers of the caller's scratch scope `tmp`"""
        n, L = self.shape
        isz = self.dtype.itemsize
        d_invq, d_idx, d_val = tmp(nq * isz), tmp(nq * k * 8), tmp(nq * k * isz)
        self._row_inv_norms(d_q, nq, d_invq.ptr)
        if self.dtype != np.float32:
            self.ctx.cosine_topk_f64_dev(d_q, nq, self._db.ptr, n, L, d_invq.ptr, self._inv.ptr, int(k), d_idx.ptr, d_val.ptr)
        elif nq >= 512:           # as the host entry point: the filtered retrieval gives the same lists faster, and declines what does not qualify
            self.ctx.cosine_topk_filtered_dev(d_q, nq, self._db.ptr, n, L, d_invq.ptr, self._inv.ptr, int(k), d_idx.ptr, d_val.ptr)
        else:
            self.ctx.cosine_topk_dev(d_q, nq, self._db.ptr, n, L, d_invq.ptr, self._inv.ptr, int(k), 0, False, d_idx.ptr, d_val.ptr)
        return d_invq, d_idx, d_val

    def _rank_dev_range(self, tmp, d_q: int, nq: int, k: int, lo: int, hi: int):
        """`_rank_dev_buffers` of a float32 index against the resident rows [lo, hi) alone, 1 <= k <= hi - lo: the same entry points,
        the same 512-query rule, the norms at _inv + lo -> (idx int64 (nq, k) counted FROM lo, val (nq, k)), DeviceBuffers of `tmp`.
        No entry point refuses the base of a sub-range: with L % 4 == 0 every row starts on 16 bytes, and any other L takes the
        generic GEMM for every call, whatever the base (the filtered entry declines such rows and ranks them by the plain one), so a
        score has the bits it has in a ranking of all rows and no aligned copy is staged.  `_last_range_stats`: what the filtered
        entry reported for this call, None where the plain one ranked."""
        n, L = self.shape
        if self.dtype != np.float32 or not 0 <= lo < hi <= n or not 1 <= k <= hi - lo:
            raise ValueError(f"a sub-range ranking needs a float32 index, 0 <= lo < hi <= {n} and 1 <= k <= hi - lo")
        d_invq, d_idx, d_val = tmp(nq * 4), tmp(nq * k * 8), tmp(nq * k * 4)
        self._row_inv_norms(d_q, nq, d_invq.ptr)
        d_rows, d_inv = self._db.ptr + lo * L * 4, self._inv.ptr + lo * 4
        self._last_range_stats = None
        if nq >= 512:
            self._last_range_stats = self.ctx.cosine_topk_filtered_dev(d_q, nq, d_rows, hi - lo, L, d_invq.ptr, d_inv, int(k), d_idx.ptr,
                                                                       d_val.ptr)
        else:
            self.ctx.cosine_topk_dev(d_q, nq, d_rows, hi - lo, L, d_invq.ptr, d_inv, int(k), 0, False, d_idx.ptr, d_val.ptr)
        return d_idx, d_val

    def _rank_dev(self, d_q: int, nq: int, k: int, want_inv: bool = False):
        """`rank` of nq rows of the index's dtype that are on the device (raw pointer) -> (idx, val[, 1 / ||q|| (nq,)])."""
        dt = self.dtype
        with self.ctx.scratch() as tmp:
            d_invq, d_idx, d_val = self._rank_dev_buffers(tmp, d_q, nq, k)
            out = d_idx.download((nq, k), np.int64), d_val.download((nq, k), dt)
            return out + (d_invq.download((nq,), dt),) if want_inv else out

    def _inv_norms_dev(self, d_q: int, nq: int) -> np.ndarray:
        """1 / ||row|| of nq device rows of the index's dtype, by the kernel the rankings use -> host (nq,)"""
        with self.ctx.scratch() as tmp:
            d_inv = tmp(nq * self.dtype.itemsize)
            self._row_inv_norms(d_q, nq, d_inv.ptr)
            return d_inv.download((nq,), self.dtype)

    def subset(self, allowed):
        """A pvsim.Subset of this index (float32 only): `allowed` is a 1-d integer array of indices in any order, a boolean mask of
        length N, or an iterable of paths.  Pass it to `rank(..., allowed=)` as often as needed; it is a snapshot and refuses once rows
        were added or removed."""
        from .subset import Subset
        return Subset(self, allowed)

    def rank(self, query_vecs: np.ndarray, k: int, allowed=None, subset_path: str = "auto"):
        """-> (idx (nq, k) int64, val (nq, k)) of the queries against the resident database; 1 <= k <= N.
        `allowed` (a pvsim.Subset of this index, or what `subset` takes): the same ranking with every row outside the set deleted,
        1 <= k <= |S| <= N and k <= 1024, float32 index and queries only; `subset_path` "auto", "mask" or "listed" pins how it is
        computed, never what; `last_subset_stats` holds what the device reported."""
        if allowed is not None:
            from .subset import rank_subset
            return rank_subset(self, query_vecs, k, allowed, subset_path)
        q = np.asarray(query_vecs)
        if q.ndim != 2 or q.shape[1] != self.shape[1]:
            raise ValueError("query and database dimensions differ")
        if self.dtype == np.float32 and q.dtype != np.float32:           # mixed dtypes: float64 scores from the host copies
            return self.ctx.cosine_topk_f64(q, self._host, int(k))
        with self.ctx.scratch() as tmp:
            return self._rank_dev(tmp.upload(np.ascontiguousarray(q, dtype=self.dtype)).ptr, q.shape[0], int(k))

    # ---- threshold search: everything at least this similar (pvsim/duplicates.py)
    def _range_dev(self, tmp, d_q: int, nq: int, d_invq: int, threshold, limit, path: str, upper: bool):
        """The threshold join of nq device rows (with their norms) against the resident rows, the triples left on the device:
        -> (rows int64, cols int64, vals float32: DeviceBuffers of the scratch scope `tmp`, total, stats).  The first call offers
        max(4096, 4 nq) entries (`limit` if that is smaller); a CapacityError is answered by ONE retry at the reported total, unless
        the total exceeds `limit`: then it is raised again, carrying the total."""
        from . import _ffi
        from .duplicates import _path_code
        n, L = self.shape
        flags = _ffi.RANGE_UPPER if upper else 0
        cap = max(4096, 4 * nq) if limit is None else min(max(4096, 4 * nq), int(limit))
        for attempt in (0, 1):
            bufs = tmp(max(cap, 1) * 8), tmp(max(cap, 1) * 8), tmp(max(cap, 1) * 4)
            try:
                total, stats = self.ctx.cosine_range_dev(d_q, nq, self._db.ptr, n, L, d_invq, self._inv.ptr, threshold, cap, bufs[0].ptr,
                                                         bufs[1].ptr, bufs[2].ptr, flags=flags, path=_path_code(path))
                return bufs + (total, dict(stats, retried=bool(attempt), threshold=float(threshold)))
            except _ffi.CapacityError as e:
                total = e.args[1]
                if attempt or (limit is not None and total > int(limit)):
                    raise _ffi.CapacityError(f"{total} results exceed the limit of {cap if limit is None else int(limit)}", total) from None
                cap = total

    def range_search(self, query_vecs: np.ndarray, threshold: float, *, max_results=None, path: str = "auto"):
        """Every database row whose cosine with a query is at least `threshold` (rounded once to float32; the comparison is in
        float32 on the score `rank` reports) -> CSR (indptr int64 (nq + 1,), indices int64, scores float32): query i owns the
        entries indptr[i]:indptr[i + 1], ordered (score descending, index ascending) as every ranking.  `max_results` bounds the
        total over all queries: more raises CapacityError carrying the total (args[1]).  path: "auto", "exact" (float32 panels) or
        "filtered" (fp16 prefilter + exact re-score); the result is the same bytes.  `last_range_stats` holds what the device reported."""
        from .duplicates import _check_index, _check_limit, _check_threshold
        _check_index(self)
        t = _check_threshold(threshold)
        limit = _check_limit("max_results", max_results)
        q = np.asarray(query_vecs)
        if q.ndim != 2 or q.shape[1] != self.shape[1]:
            raise ValueError("query and database dimensions differ")
        if q.dtype != np.float32:
            raise TypeError(f"a threshold search scores in float32: float32 queries on a float32 DeviceIndex, got {q.dtype}")
        nq, n = q.shape[0], self.shape[0]
        if nq == 0 or n == 0:
            self.last_range_stats = {"threshold": float(t)}
            return np.zeros(nq + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        with self.ctx.scratch() as tmp:
            d_q, d_invq = tmp.upload(np.ascontiguousarray(q)), tmp(nq * 4)
            self._row_inv_norms(d_q.ptr, nq, d_invq.ptr)
            d_row, d_col, d_val, total, self.last_range_stats = self._range_dev(tmp, d_q.ptr, nq, d_invq.ptr, t, limit, path, False)
            row, col, val = (d_row.download((total,), np.int64), d_col.download((total,), np.int64), d_val.download((total,), np.float32))
        order = np.lexsort((col, -val, row))                 # one stable sort; -0 and +0 tie and the index decides
        indptr = np.zeros(nq + 1, np.int64)
        np.cumsum(np.bincount(row, minlength=nq), out=indptr[1:])
        return indptr, col[order], val[order]

    def similar_pairs(self, threshold: float, *, max_pairs=None, path: str = "auto"):
        """The self-join: every pair of rows i < j whose cosine is at least `threshold` -> (i int64, j int64, score float32) in
        (i, j) order.  `max_pairs` bounds the number of pairs: more raises CapacityError carrying the total.  `path` as range_search."""
        from .duplicates import _check_index, _check_limit, _check_threshold
        _check_index(self)
        t = _check_threshold(threshold)
        limit = _check_limit("max_pairs", max_pairs)
        n = self.shape[0]
        if n == 0:
            self.last_range_stats = {"threshold": float(t)}
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        with self.ctx.scratch() as tmp:
            d_row, d_col, d_val, total, self.last_range_stats = self._range_dev(tmp, self._db.ptr, n, self._inv.ptr, t, limit, path, True)
            row, col, val = (d_row.download((total,), np.int64), d_col.download((total,), np.int64), d_val.download((total,), np.float32))
        order = np.lexsort((col, row))
        return row[order], col[order], val[order]

    # ---- query expansion and database-side augmentation (pvsim/expand.py)
    def _list_weights(self, idx, val, scheme, alpha):
        """weights of list entries `idx` with similarities `val`: expansion_weights(...) * inv_norms[idx], 0 on the -1 slots"""
        from .expand import expansion_weights
        inv = self.inv_norms
        filled = idx >= 0
        w = expansion_weights(val, scheme, alpha) * inv[np.where(filled, idx, 0)] if inv.size else np.zeros_like(val)
        return np.ascontiguousarray(np.where(filled, w, self._hbuf.dtype.type(0)))

    def _combine(self, d_self, w_self, idx, w, d_out):
        """pvs_combine_rows_dev of the resident rows: lists and weights go up, the rows stay where they are"""
        n, r = idx.shape
        N, L = self.shape
        with self.ctx.scratch() as tmp:
            d_w_self, d_idx, d_w = tmp.upload(w_self), tmp.upload(idx), tmp.upload(w)
            self.ctx.combine_rows_dev(self._db.ptr, N, L, self.dtype == np.float64, d_self, d_w_self.ptr,
                                      d_idx.ptr if r else None, d_w.ptr if r else None, n, r, d_out)

    def rank_expanded(self, query_vecs: np.ndarray, k: int, qe, members=None, return_queries: bool = False):
        """`rank` after query expansion `qe` (pvsim.expand.QueryExpansion): the queries are ranked, each is replaced by
        qe.query_weight * q / |q| + sum_j w_j x_j / |x_j| over the first min(qe.n, N) entries x_j of its list (w_j from
        expansion_weights of the list's scores), and the new rows are ranked; with qe.passes > 1 this repeats from the lists of the
        new rows, always adding to the original query.  The sums run on the device, against the resident rows.
        `members`: (nq, m) int64 database indices, -1 for an empty slot, that replace the first list (verified results, say); their
        scores (only the "alpha" scheme reads them) are looked up in the complete first ranking.
        -> (idx (nq, k), val (nq, k)), and the expanded queries (nq, L) behind them with return_queries.
        A float64 query against a float32 index raises TypeError: expansion works in the index's dtype."""
        from .expand import QueryExpansion
        if not isinstance(qe, QueryExpansion):
            raise TypeError("qe must be a pvsim.expand.QueryExpansion")
        q = np.asarray(query_vecs)
        N, L = self.shape
        dt = self.dtype
        if q.ndim != 2 or q.shape[1] != L:
            raise ValueError("query and database dimensions differ")
        if dt == np.float32 and q.dtype != np.float32:
            raise TypeError("query expansion works in the index's dtype: a float32 index needs float32 queries")
        if not 1 <= int(k) <= N:
            raise ValueError(f"need 1 <= k <= N (k = {k}, N = {N})")
        q = np.ascontiguousarray(q, dtype=dt)
        nq = q.shape[0]
        if members is not None:
            members = np.ascontiguousarray(members, dtype=np.int64)
            if members.ndim != 2 or members.shape[0] != nq:
                raise ValueError("members must be an (nq, m) array of database indices")
            if members.size and (members.min() < -1 or members.max() >= N):
                raise ValueError("members must be database indices in [0, N), or -1 for an empty slot")
        if nq == 0:
            out = (np.zeros((0, int(k)), np.int64), np.zeros((0, int(k)), dt))
            return out + (q,) if return_queries else out
        n1 = min(qe.n, N)
        with self.ctx.scratch() as tmp:
            d_q, d_e = tmp.upload(q), tmp(q.nbytes)
            if members is None:
                idx, val, inv_q = self._rank_dev(d_q.ptr, nq, n1, want_inv=True)
            elif qe.scheme == "alpha":                                   # the members' scores: from the complete ranking
                full_idx, full_val, inv_q = self._rank_dev(d_q.ptr, nq, N, want_inv=True)
                score_of = np.empty((nq, N), dt)
                np.put_along_axis(score_of, full_idx, full_val, axis=1)
                idx, val = members, np.take_along_axis(score_of, np.where(members >= 0, members, 0), axis=1)
            else:
                inv_q = self._inv_norms_dev(d_q.ptr, nq)
                idx, val = members, np.zeros(members.shape, dt)
            w_self = dt.type(qe.query_weight) * inv_q
            for p in range(qe.passes):
                self._combine(d_q.ptr, w_self, idx, self._list_weights(idx, val, qe.scheme, qe.alpha), d_e.ptr)
                if p + 1 < qe.passes:
                    idx, val = self._rank_dev(d_e.ptr, nq, n1)
            out = self._rank_dev(d_e.ptr, nq, int(k))
            return out + (d_e.download((nq, L), dt),) if return_queries else out

    def augmented(self, r: int = 10, scheme: str = "linear", alpha: int = 3, block: int = 4096) -> "DeviceIndex":
        """Database-side augmentation: a new DeviceIndex with the same paths in the same order, whose row i is
        x_i / |x_i| + sum_j w_j x_j / |x_j| over the min(r, N - 1) nearest other rows of this index (w_j from expansion_weights
        of their similarities to row i; "linear" falls from 1 to 1 / r with the rank).  Rows are ranked `block` at a time against
        the whole index; only the lists and weights cross to the host.  This index is left as it is.  The result is a separate
        index: a later `add` or `remove` on this one does not reach it."""
        from .expand import _check_count, _check_scheme, drop_self
        _check_count("r", r)
        _check_count("block", block)
        _check_scheme(scheme, alpha)
        N, L = self.shape
        dt = self.dtype
        d_new = self.ctx.buffer(N * L * dt.itemsize)
        if N and L:
            kk = min(int(r), N - 1) + 1
            inv = self.inv_norms
            for b0 in range(0, N, int(block)):
                b1 = min(N, b0 + int(block))
                d_rows = self._db.ptr + b0 * L * dt.itemsize
                idx, val = drop_self(*self._rank_dev(d_rows, b1 - b0, kk), np.arange(b0, b1))
                self._combine(d_rows, inv[b0:b1], idx, self._list_weights(idx, val, scheme, alpha), d_new.ptr + b0 * L * dt.itemsize)
        return DeviceIndex._from_device(self._paths, d_new, N, L, dt, self.ctx)

    def close(self):
        for b in (self._db, self._inv):
            b.free()
