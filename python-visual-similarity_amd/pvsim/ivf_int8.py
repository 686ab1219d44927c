"""Inverted lists over the int8 code rows: sub-linear search with the int8 score itself.

An `Int8Index` reads every code row for every query.  An `IVFInt8Index` holds the same bytes per image plus 4 for the original id,
cut into `nlist` inverted lists: a query scores the rows of its `nprobe` best lists, about nprobe / nlist of the index.  Nothing is
approximated twice: the centroids are code rows themselves, the list of a row and the probes of a query are both rankings by
pvs_sq8_topk_dev against the centroid codes, and every reported score is, bit for bit, the score `Int8Index.rank` reports for that
pair.  `rank(q, k, nprobe=nlist)` equals `Int8Index.rank(q, k)` on the same rows byte for byte.  The definitions are in include/pvsim.h;
tests/ivf_sq8_numpy.py restates them."""
from __future__ import annotations

import numpy as np

from .compact import MAX_IVF_K, MAX_NLIST, MAX_NPROBE, _check_nlist, _sort_into_lists
from .index import DeviceIndex, _PathLedger, _keep_positions
from .quantized import _CHUNK_BYTES, Int8Index, _all_finite, _check_length, _f32_rows, padded_length

__all__ = ["IVFInt8Index", "save_ivf_int8_arrays", "load_ivf_int8_arrays"]

KIND = "ivf_int8_index"
COMBINE_MEMBERS = 4096           # members of a list that one pass of pvs_combine_rows_dev adds to its centroid


# ------------------------------------------------------------------------------------------------ persistence (no device needed)
def save_ivf_int8_arrays(path: str, paths, codes, factors, ids, list_off, centroids, L: int) -> None:
    """One plain .npz (numpy.load(allow_pickle=False)): kind, paths, codes int8 (N, L) without the padding and factors float32 (N,) in
    STORED order, ids int32 (N,), list_off int64 (nlist + 1,), centroids float32 (nlist, L), L."""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    factors = np.ascontiguousarray(factors, dtype=np.float32)
    paths = [str(p) for p in paths]
    n, L = len(paths), int(L)
    if codes.ndim != 2 or codes.shape != (n, L) or factors.shape != (n,):
        raise ValueError(f"codes must be int8 ({n}, {L}) and factors float32 ({n},), got {codes.shape} and {factors.shape}")
    ids, list_off, centroids = _check_lists(n, L, ids, list_off, centroids)
    np.savez(path, kind=KIND, paths=np.array(paths, dtype=np.str_), codes=codes, factors=factors, ids=ids, list_off=list_off,
             centroids=centroids, L=np.int64(L))


def load_ivf_int8_arrays(path: str) -> dict:
    """-> dict(paths, codes, factors, ids, list_off, centroids, L); a file of another kind is a ValueError"""
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
        if "kind" not in z.files or str(z["kind"]) != KIND:
            raise ValueError(f"{path}: not an IVF int8 index file")
        out = dict(paths=[str(p) for p in z["paths"]], codes=z["codes"], factors=z["factors"], ids=z["ids"], list_off=z["list_off"],
                   centroids=z["centroids"], L=int(z["L"]))
    n, L = len(out["paths"]), out["L"]
    if out["codes"].dtype != np.int8 or out["codes"].shape != (n, L) or out["factors"].dtype != np.float32 or out["factors"].shape != (n,):
        raise ValueError(f"{path}: the arrays of the IVF int8 index file do not fit each other")
    out["ids"], out["list_off"], out["centroids"] = _check_lists(n, L, out["ids"], out["list_off"], out["centroids"])
    return out


def _check_centroids(centroids, L: int) -> np.ndarray:
    cent = _f32_rows(centroids, "centroids")
    if cent.shape[1] != L or not 1 <= cent.shape[0] <= MAX_NLIST:
        raise ValueError(f"centroids must be float32 (nlist, {L}) with 1 <= nlist <= {MAX_NLIST}, got {cent.shape}")
    return cent


def _check_lists(n: int, L: int, ids, list_off, centroids):
    """the inverted-list arrays of n stored rows -> (ids int32, list_off int64, centroids float32), checked against each other"""
    cent = _check_centroids(centroids, L)
    off = np.asarray(list_off)
    if off.dtype.kind not in "iu" or off.shape != (cent.shape[0] + 1,):
        raise ValueError(f"list_off must be ({cent.shape[0] + 1},) integers, got {off.dtype} {off.shape}")
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError(f"list_off must rise from 0 to {n} without decreasing")
    ids = np.asarray(ids)
    if ids.dtype.kind not in "iu" or ids.shape != (n,):
        raise ValueError(f"ids must be ({n},) integers, got {ids.dtype} {ids.shape}")
    if n >= 2 ** 31:
        raise ValueError(f"an IVF int8 index holds fewer than 2^31 rows, got {n}")
    if n and not np.array_equal(np.sort(ids), np.arange(n)):
        raise ValueError(f"ids must be a permutation of 0 .. {n - 1}")
    return np.ascontiguousarray(ids, dtype=np.int32), off, cent


def _draw(n: int, train, nlist: int, rng):
    """-> (sample: sorted int64 indices of the training rows, init: positions in the sample of the nlist initial centroids).  `train`
    None takes every row; an integer draws that many distinct rows with the seeded generator.  The initial centroids are nlist
    distinct sample rows drawn next."""
    if train is None:
        sample = np.arange(n, dtype=np.int64)
    else:
        sample = np.sort(rng.choice(n, int(train), replace=False)).astype(np.int64)
    init = np.asarray(rng.choice(sample.size, nlist, replace=False), dtype=np.int64)
    return sample, init


def _check_train(train, n: int):
    if train is None:
        return n
    if isinstance(train, bool) or not isinstance(train, (int, np.integer)) or not 1 <= train <= n:
        raise ValueError(f"train must be None (all rows) or the number of training rows, an integer with 1 <= train <= {n}, got {train!r}")
    return int(train)


# ------------------------------------------------------------------------------------------------ index
class IVFInt8Index:
    """Paths + int8 codes (N, ld) + float32 row factors (N,) + original ids int32 (N,) in (list, original index) order on the device,
    the list offsets on the device and the host, and the centroids as float32 rows (host) and as code rows (device).

    `build(source, centroids)` assigns the rows of a {path: float32 vector} mapping, a float32 DeviceIndex or an Int8Index to the lists
    of given centroids; `fit(source, nlist)` trains the centroids first (spherical k-means on the codes' own score).  `rank(q, k,
    nprobe)` scans the nprobe best lists of each query.  `add`, `remove` / `del index[path]` and `reserve` change the index without
    a rebuild: the centroids are never retrained, and after any sequence of updates every array equals, byte for
    byte, that of a `build` from the surviving rows in surviving order with the same centroids."""

    # ---- construction
    @classmethod
    def build(cls, source, centroids, ctx=None) -> "IVFInt8Index":
        """Rows -> codes (pvs_sq8_encode_dev; the codes of an Int8Index are taken as they are), centroids -> centroid codes, the list of
        every row = pvs_sq8_topk_dev with k = 1 against the centroid codes, then the rows sorted by (list, original index)."""
        from .engine import default_context
        flat = resident = mat = None                 # the three kinds of source: an Int8Index, a float32 DeviceIndex, host rows
        if isinstance(source, Int8Index):
            flat, ctx, paths, L = source, ctx or source.ctx, source.keys(), source.shape[1]
        elif isinstance(source, DeviceIndex):
            if source.dtype != np.float32:
                raise TypeError("the DeviceIndex is float64: the int8 codes are made from float32 rows")
            if not _all_finite(source.matrix):
                raise ValueError("database holds a NaN or an infinity: the int8 codes are defined for finite rows only")
            resident, ctx, paths, L = source, ctx or source.ctx, list(source.keys()), source.shape[1]
        else:
            paths = [str(p) for p in source.keys()]
            mat = np.array(list(source.values()))
            if mat.ndim != 2:
                raise ValueError("IVFInt8Index needs one vector of the same length per entry")
            mat = _f32_rows(mat, "database")
            ctx, L = ctx or default_context(), mat.shape[1]
        L = _check_length(L)
        cent = _check_centroids(centroids, L)
        n = len(paths)
        if n >= 2 ** 31:
            raise ValueError(f"an IVF int8 index holds fewer than 2^31 rows, got {n}")
        self = cls.__new__(cls)
        self._init_empty(paths, L, cent, ctx)
        ld = self._ld
        with ctx.scratch() as tmp:
            if flat is not None:
                d_codes, d_inv = flat._codes.ptr, flat._inv.ptr
            else:
                d_codes, d_inv = tmp(max(n * ld, 16)).ptr, tmp(max(n * 4, 16)).ptr
                self._encode_rows(resident, mat, d_codes, d_inv)
            ids, list_off = _sort_into_lists(self._assign(d_codes, d_inv, n), self.nlist)
            self._codes, self._inv = ctx.buffer(max(n * ld, 16)), ctx.buffer(max(n * 4, 16))
            if n:
                d_order = tmp.upload(ids.astype(np.int64))
                ctx.graph_gather_rows_dev(d_codes, n, ld, d_order.ptr, n, self._codes.ptr)
                ctx.graph_gather_rows_dev(d_inv, n, 4, d_order.ptr, n, self._inv.ptr)
                ctx.sync()
        self._set_lists(ids, list_off)
        return self

    @classmethod
    def fit(cls, source, nlist: int, train=None, random_state=None, max_iter: int = 10, ctx=None) -> "IVFInt8Index":
        """Train `nlist` centroids on `train` rows of `source` (None: all of them; an integer: that many, drawn with the seeded
        generator), then `build`.  `source` is a mapping or a float32 DeviceIndex; an Int8Index keeps no float rows to train on.
        Spherical k-means composed from existing entry points: the sample and its inverse norms, nlist distinct
        sample rows as initial centroids, then per iteration the centroids' codes, the label of every sample row by pvs_sq8_topk_dev
        with k = 1, and the new centroid of a list = sum of inv_norm_i x_i over its members i ascending by pvs_combine_rows_dev, an
        empty list keeping its centroid; it stops when no label changes or after max_iter iterations."""
        from .engine import default_context
        from .learn import _rng
        if isinstance(source, Int8Index):
            raise TypeError("fit needs the float32 rows to train on: pass a mapping or a float32 DeviceIndex, or train elsewhere and "
                            "call IVFInt8Index.build(int8_index, centroids)")
        _check_nlist(nlist, nlist, 0)                # the type and range, before anything is computed
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
            raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
        own = None
        if isinstance(source, DeviceIndex):
            if source.dtype != np.float32:
                raise TypeError("the DeviceIndex is float64: the int8 codes are made from float32 rows")
            resident, ctx = source, ctx or source.ctx
        else:
            mat = np.array(list(source.values()))
            if mat.ndim != 2:
                raise ValueError("IVFInt8Index needs one vector of the same length per entry")
            _f32_rows(mat, "database")
            ctx = ctx or default_context()
            resident = own = DeviceIndex(source, ctx)            # the rows go up once, for the training and the build
        try:
            n, L = resident.shape
            _check_length(L)
            if not _all_finite(resident.matrix):
                raise ValueError("database holds a NaN or an infinity: the int8 codes are defined for finite rows only")
            nt = _check_train(train, n)
            nlist = _check_nlist(nlist, nt, n)
            sample, init = _draw(n, train, nlist, _rng(random_state))
            cent = _train(ctx, resident._db.ptr, n, L, sample, init, int(max_iter))
            return cls.build(resident, cent, ctx)
        finally:
            if own is not None:
                own.close()

    @classmethod
    def _from_arrays(cls, paths, codes, factors, ids, list_off, centroids, L, ctx=None) -> "IVFInt8Index":
        """An index over given arrays in stored order: they go up as they are, only the centroids are encoded again"""
        from .engine import default_context
        L = _check_length(L)
        ids, list_off, cent = _check_lists(len(paths), L, ids, list_off, centroids)
        self = cls.__new__(cls)
        self._init_empty(paths, L, cent, ctx or default_context())
        n = len(paths)
        self._codes, self._inv = self.ctx.buffer(max(n * self._ld, 16)), self.ctx.buffer(max(n * 4, 16))
        if n:
            padded = np.zeros((n, self._ld), np.int8)
            padded[:, :L] = codes
            self._codes.upload(padded)
            self._inv.upload(np.ascontiguousarray(factors, dtype=np.float32))
        self._set_lists(ids, list_off)
        return self

    def _init_empty(self, paths, L, centroids, ctx):
        self.ctx, self._L, self._ld = ctx, int(L), padded_length(L)
        self._ledger = _PathLedger([str(p) for p in paths])
        if len(set(self._ledger.paths)) != len(self._ledger.paths):
            raise ValueError("a path is named twice")
        self.modifications = 0
        self.last_scan = None
        self._centroids = centroids
        nlist = centroids.shape[0]
        self._cent_codes, self._cent_inv = ctx.buffer(nlist * self._ld), ctx.buffer(max(nlist * 4, 16))
        with ctx.scratch() as tmp:
            ctx.sq8_encode_dev(tmp.upload(centroids).ptr, nlist, self._L, self._cent_codes.ptr, self._cent_inv.ptr)
            ctx.sync()
        self._codes = self._inv = self._ids = self._d_list_off = None

    def _set_lists(self, ids: np.ndarray, list_off: np.ndarray) -> None:
        """upload ids and list_off; the host keeps list_off (every call sizes its launches from it) and the ids it was given"""
        ctx, n = self.ctx, len(self)
        self._ids = ctx.buffer(max(n * 4, 16))
        if n:
            self._ids.upload(np.ascontiguousarray(ids, dtype=np.int32))
        self._list_off = np.ascontiguousarray(list_off, dtype=np.int64)
        self._d_list_off = ctx.buffer(self._list_off.nbytes).upload(self._list_off)
        self._ids_host = np.ascontiguousarray(ids, dtype=np.int32)

    def _encode_rows(self, resident, mat, d_codes: int, d_inv: int) -> None:
        """the float32 rows of a DeviceIndex (read in place) or of a host matrix (a chunk at a time) -> codes and factors at the raw
        device addresses d_codes, d_inv"""
        ctx, L, ld = self.ctx, self._L, self._ld
        if resident is not None:
            n = resident.shape[0]
            if n:
                ctx.sq8_encode_dev(resident._db.ptr, n, L, d_codes, d_inv)
                ctx.sync()
            return
        step = max(1, _CHUNK_BYTES // (4 * L))
        for r0 in range(0, mat.shape[0], step):
            rn = min(step, mat.shape[0] - r0)
            with ctx.scratch() as tmp:
                ctx.sq8_encode_dev(tmp.upload(mat[r0:r0 + rn]).ptr, rn, L, d_codes + r0 * ld, d_inv + r0 * 4)
                ctx.sync()

    def _assign(self, d_codes: int, d_inv: int, n: int) -> np.ndarray:
        """the list of each of n code rows at the raw device addresses -> host int64 (n,)"""
        if n == 0:
            return np.zeros(0, np.int64)
        return _labels(self.ctx, d_codes, d_inv, n, self._cent_codes.ptr, self._cent_inv.ptr, self.nlist, self._L)

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
    def nlist(self) -> int:
        return self._centroids.shape[0]

    @property
    def centroids(self) -> np.ndarray:
        """the float32 centroid rows (nlist, L) as given or trained"""
        return self._centroids

    @property
    def list_sizes(self) -> np.ndarray:
        """rows per inverted list, int64 (nlist,)"""
        return np.diff(self._list_off)

    @property
    def _ids_stored(self) -> np.ndarray:
        """host copy of the stored rows' original indices: downloaded when `save` or a check needs it after an update"""
        if self._ids_host is None:
            n = len(self)
            self._ids_host = self._ids.download((n,), np.int32) if n else np.zeros(0, np.int32)
        return self._ids_host

    @property
    def nbytes_breakdown(self) -> dict:
        n, nlist = len(self), self.nlist
        return {"codes": n * self._ld, "factors": n * 4, "ids": n * 4, "list_off": (nlist + 1) * 8, "centroid_codes": nlist * self._ld,
                "centroid_factors": nlist * 4}

    @property
    def nbytes(self) -> int:
        """device bytes: N (64 ceil(L / 64) + 8) for the rows, plus the centroid codes and the offsets"""
        return int(sum(self.nbytes_breakdown.values()))

    def _download(self):
        """-> (codes int8 (N, ld) with the padding, factors float32 (N,), ids int32 (N,)) in stored order, list_off int64"""
        n = len(self)
        if n == 0:
            return np.zeros((0, self._ld), np.int8), np.zeros(0, np.float32), np.zeros(0, np.int32), self._list_off.copy()
        return (self._codes.download((n, self._ld), np.int8), self._inv.download((n,), np.float32), self._ids_stored.copy(),
                self._list_off.copy())

    # ---- updates
    def reserve(self, n: int) -> None:
        """Every insert merges the stored arrays into fresh buffers sized for the result (the storage of section 14), so there is no
        capacity to grow ahead of time: the call checks n and changes nothing, as on an IVFCompactIndex without kept rows."""
        if isinstance(n, bool) or int(n) != n or n < 0:
            raise ValueError(f"reserve takes a number of rows >= 0, got {n!r}")
        if int(n) >= 2 ** 31:
            raise ValueError(f"an IVF int8 index holds fewer than 2^31 rows, got {n}")

    def _swap_stored(self, codes, inv, ids, off, list_off) -> None:
        for name, new in (("_codes", codes), ("_inv", inv), ("_ids", ids), ("_d_list_off", off)):
            getattr(self, name).free()
            setattr(self, name, new)
        self._list_off, self._ids_host = np.ascontiguousarray(list_off, dtype=np.int64), None

    def add(self, source) -> None:
        """Append new images: `source` is {path: float32 vector of L} or a float32 DeviceIndex whose resident rows are read in place.
        They get the original indices N, N + 1, ... in the order given and join the list of their best centroid.  A path that is
        already indexed is a ValueError, raised before anything changes.  The centroids stay as they are."""
        resident = source if isinstance(source, DeviceIndex) else None
        paths = [str(p) for p in source.keys()]
        if not paths:
            return
        self._ledger.check_new(paths)
        if resident is not None:
            if resident.dtype != np.float32:
                raise TypeError("an IVF int8 index takes float32 vectors, the DeviceIndex is float64")
            mat = resident.matrix
        else:
            mat = np.array(list(source.values()))
        if mat.ndim != 2 or mat.shape[1] != self._L:
            raise ValueError(f"new vectors must have the index's length {self._L}, got an array of shape {mat.shape}")
        mat = _f32_rows(mat, "new vectors")
        ctx, n, b, ld, nlist = self.ctx, len(self), len(paths), self._ld, self.nlist
        if n + b >= 2 ** 31:
            raise ValueError(f"an IVF int8 index holds fewer than 2^31 rows, got {n + b}")
        with ctx.scratch() as tmp:
            d_codes, d_inv = tmp(b * ld), tmp(b * 4)
            self._encode_rows(resident, mat, d_codes.ptr, d_inv.ptr)
            perm, new_off = _sort_into_lists(self._assign(d_codes.ptr, d_inv.ptr, b), nlist)
            d_perm, d_new_off = tmp.upload(perm), tmp.upload(new_off)
            out = [tmp(max(nbytes, 16)) for nbytes in ((n + b) * ld, (n + b) * 4, (n + b) * 4, (nlist + 1) * 8)]
            ctx.ivf_insert_dev(ld, nlist, self._codes.ptr, self._inv.ptr, self._ids.ptr, self._d_list_off.ptr, self._list_off,
                               d_codes.ptr, d_inv.ptr, d_new_off.ptr, new_off, d_perm.ptr, *(o.ptr for o in out))
            ctx.sync()
            self._swap_stored(*(tmp.keep(o) for o in out), self._list_off + new_off)
        self._ledger.append(paths)
        self.modifications += 1

    def remove(self, paths) -> None:
        """The named images leave, the others keep their relative order; the original index of a survivor falls by the number of
        removed rows before it.  An unknown path is a KeyError, a path named twice a ValueError, both raised before anything changes."""
        idx = self._ledger.removed_indices([paths] if isinstance(paths, str) else [str(p) for p in paths])
        if idx.size == 0:
            return
        ctx, n, ld, nlist = self.ctx, len(self), self._ld, self.nlist
        left = n - idx.size
        with ctx.scratch() as tmp:
            keep, pos = _keep_positions(tmp, idx, n)
            out = [tmp(max(nbytes, 16)) for nbytes in (left * ld, left * 4, left * 4, (nlist + 1) * 8)]
            ctx.ivf_remove_dev(ld, nlist, n, self._codes.ptr, self._inv.ptr, self._ids.ptr, self._d_list_off.ptr, keep.ptr, pos.ptr,
                               *(o.ptr for o in out))
            list_off = out[3].download((nlist + 1,), np.int64)
            self._swap_stored(*(tmp.keep(o) for o in out), list_off)
        self._ledger.remove(idx)
        self.modifications += 1

    def __delitem__(self, path) -> None:
        self.remove([path])

    # ---- search
    def _check_rank_args(self, k, nprobe):
        n, most = len(self), min(self.nlist, MAX_NPROBE)
        if isinstance(nprobe, bool) or nprobe is None or int(nprobe) != nprobe or not 1 <= nprobe <= most:
            raise ValueError(f"nprobe must be an integer with 1 <= nprobe <= {most} (min(nlist, {MAX_NPROBE})), got {nprobe!r}")
        if isinstance(k, bool) or k is None or int(k) != k or not 1 <= k <= min(n, MAX_IVF_K):
            raise ValueError(f"k must be an integer with 1 <= k <= {min(n, MAX_IVF_K)} (min(N, {MAX_IVF_K})), got {k!r}")
        return int(k), int(nprobe)

    def rank(self, query_vecs, k: int, nprobe: int, slice_rows: int = 0, scan: str = "queries", query_block: int = 0):
        """-> (idx (nq, k) int64, val (nq, k) float32): the queries are quantised by the rule of the rows, the `nprobe` best lists of
        each are scanned and ranked by (score descending, original index ascending); slots the probed lists cannot fill are -1 /
        -inf.  1 <= k <= min(N, 1024), 1 <= nprobe <= min(nlist, 1024).

        `scan` chooses who computes the candidate scores, never what they are: "queries" walks the probed rows once per query,
        "lists" groups the queries of a block by list and scores every row tile of a probed list against its group on the int8
        matrix pipe, reading a probed row once per query block: the choice for batches.  The two give the same
        bytes.  `slice_rows` (with "queries") and `query_block` (with "lists") pin how the scan is cut, never what it gives."""
        if scan not in ("queries", "lists"):
            raise ValueError(f'scan must be "queries" or "lists", got {scan!r}')
        if scan == "lists" and slice_rows != 0:
            raise ValueError('slice_rows cuts the scan by query: it does not go with scan="lists" (query_block does)')
        if scan == "queries" and query_block != 0:
            raise ValueError('query_block cuts the scan by list: it does not go with scan="queries" (slice_rows does)')
        q = _f32_rows(query_vecs, "query")
        n, L = self.shape
        if q.shape[1] != L:
            raise ValueError(f"query and database dimensions differ: {q.shape[1]} vs {L}")
        k, nprobe = self._check_rank_args(k, nprobe)
        nq, ctx, nlist = q.shape[0], self.ctx, self.nlist
        if nq == 0:
            return np.zeros((0, k), np.int64), np.zeros((0, k), np.float32)
        with ctx.scratch() as tmp:
            d_q, d_qc, d_invq = tmp.upload(q), tmp(nq * self._ld), tmp(nq * 4)
            d_pidx, d_pval = tmp(nq * nprobe * 8), tmp(nq * nprobe * 4)
            d_idx, d_val = tmp(nq * k * 8), tmp(nq * k * 4)
            ctx.sq8_encode_dev(d_q.ptr, nq, L, d_qc.ptr, d_invq.ptr)
            ctx.sq8_topk_dev(d_qc.ptr, d_invq.ptr, nq, self._cent_codes.ptr, self._cent_inv.ptr, nlist, L, nprobe, 0, False, d_pidx.ptr,
                             d_pval.ptr)
            if scan == "lists":
                ctx.ivf_sq8_scan_lists_topk_dev(d_qc.ptr, d_invq.ptr, nq, L, d_pidx.ptr, nprobe, self._d_list_off.ptr, self._list_off, nlist,
                                                self._codes.ptr, self._inv.ptr, self._ids.ptr, k, d_idx.ptr, d_val.ptr,
                                                query_block=query_block)
            else:
                ctx.ivf_sq8_scan_topk_dev(d_qc.ptr, d_invq.ptr, nq, L, d_pidx.ptr, nprobe, self._d_list_off.ptr, self._list_off, nlist,
                                          self._codes.ptr, self._inv.ptr, self._ids.ptr, k, d_idx.ptr, d_val.ptr, slice_rows=slice_rows)
            out = d_idx.download((nq, k), np.int64), d_val.download((nq, k), np.float32)
            probes = d_pidx.download((nq, nprobe), np.int64)
        candidates = int(self.list_sizes[probes].sum())
        if scan == "lists":
            plan = ctx.ivf_sq8_scan_lists_plan(nq, nprobe, self._list_off, nlist, query_block)
            self.last_scan = {"scan": "lists", "W": plan["W"], "query_block": plan["query_block"], "row_tiles": plan["row_tiles"],
                              "pairs": plan["pairs"], "candidates": candidates}
        else:
            plan = ctx.ivf_sq8_scan_plan(nq, nprobe, self._list_off, nlist, slice_rows)
            self.last_scan = {"W": plan["W"], "slice_rows": plan["slice_rows"], "slices": plan["slices"], "candidates": candidates}
        return out

    # ---- persistence
    def save(self, path: str) -> None:
        codes, inv, ids, list_off = self._download()
        save_ivf_int8_arrays(path, self._ledger.paths, codes[:, :self._L], inv, ids, list_off, self._centroids, self._L)

    @classmethod
    def load(cls, path: str, ctx=None) -> "IVFInt8Index":
        a = load_ivf_int8_arrays(path)
        return cls._from_arrays(a["paths"], a["codes"], a["factors"], a["ids"], a["list_off"], a["centroids"], a["L"], ctx)

    def close(self):
        for name in ("_codes", "_inv", "_ids", "_d_list_off", "_cent_codes", "_cent_inv"):
            b = getattr(self, name, None)
            if b is not None:
                b.free()
                setattr(self, name, None)


# ------------------------------------------------------------------------------------------------ assignment and training
def _labels(ctx, d_codes: int, d_inv: int, n: int, d_cent_codes: int, d_cent_inv: int, nlist: int, L: int) -> np.ndarray:
    """the best centroid of each of n code rows: pvs_sq8_topk_dev with k = 1 -> host int64 (n,)"""
    with ctx.scratch() as tmp:
        d_l, d_v = tmp(n * 8), tmp(n * 4)
        ctx.sq8_topk_dev(d_codes, d_inv, n, d_cent_codes, d_cent_inv, nlist, L, 1, 0, False, d_l.ptr, d_v.ptr)
        return d_l.download((n,), np.int64)


def _member_lists(labels: np.ndarray, nlist: int):
    """labels (nt,) -> (members int64 (nlist, most): the sample positions of every list ascending, -1 behind them; counts (nlist,))"""
    order = np.argsort(labels, kind="stable")
    counts = np.bincount(labels, minlength=nlist)
    members = np.full((nlist, max(int(counts.max()), 1)), -1, np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    col = np.arange(labels.size) - np.repeat(first, counts)
    members[labels[order], col] = order
    return members, counts


def _train(ctx, d_rows: int, n: int, L: int, sample: np.ndarray, init: np.ndarray, max_iter: int) -> np.ndarray:
    """Spherical k-means on the sample rows of the resident float32 rows at d_rows -> centroids float32 (nlist, L)."""
    nt, nlist, ld = int(sample.size), int(init.size), padded_length(L)
    with ctx.scratch() as tmp:
        d_x, d_xinv = tmp(nt * L * 4), tmp(nt * 4)
        ctx.graph_gather_rows_dev(d_rows, n, L * 4, tmp.upload(sample).ptr, nt, d_x.ptr)
        ctx.row_inv_norms_dev(d_x.ptr, nt, L, d_xinv.ptr)
        xinv = d_xinv.download((nt,), np.float32)
        d_xc, d_xci = tmp(nt * ld), tmp(nt * 4)
        ctx.sq8_encode_dev(d_x.ptr, nt, L, d_xc.ptr, d_xci.ptr)                 # the sample's codes are made once
        d_cent, d_new = tmp(nlist * L * 4), tmp(nlist * L * 4)
        ctx.graph_gather_rows_dev(d_x.ptr, nt, L * 4, tmp.upload(init).ptr, nlist, d_cent.ptr)
        d_cc, d_ci = tmp(nlist * ld), tmp(max(nlist * 4, 16))
        prev = None
        for _ in range(max_iter):
            ctx.sq8_encode_dev(d_cent.ptr, nlist, L, d_cc.ptr, d_ci.ptr)
            labels = _labels(ctx, d_xc.ptr, d_xci.ptr, nt, d_cc.ptr, d_ci.ptr, nlist, L)
            if prev is not None and np.array_equal(labels, prev):
                break
            members, counts = _member_lists(labels, nlist)
            weights = np.where(members >= 0, xinv[np.where(members >= 0, members, 0)], np.float32(0)).astype(np.float32)
            for c0 in range(0, members.shape[1], COMBINE_MEMBERS):
                idx, w = np.ascontiguousarray(members[:, c0:c0 + COMBINE_MEMBERS]), np.ascontiguousarray(weights[:, c0:c0 + COMBINE_MEMBERS])
                with ctx.scratch() as own:
                    ctx.combine_rows_dev(d_x.ptr, nt, L, False, d_new.ptr if c0 else None, None, own.upload(idx).ptr, own.upload(w).ptr,
                                         nlist, idx.shape[1], d_new.ptr)
                    ctx.sync()
            for l in np.flatnonzero(counts == 0).tolist():                      # an empty list keeps its centroid
                ctx.copy_dev(d_new.ptr + l * L * 4, d_cent.ptr + l * L * 4, L * 4)
            d_cent, d_new = d_new, d_cent
            prev = labels
        return d_cent.download((nlist, L), np.float32)
