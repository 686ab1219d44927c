"""Compact image index: product-quantised encodings searched with asymmetric distance computation.

Jegou, Douze, Schmid, Perez (CVPR 2010; PAMI 2012) introduced VLAD together with its compression: project the encoding to a few
hundred dimensions, product-quantise it to m bytes, score a query against the codes through a per-query inner-product table, and
optionally re-rank a short list exactly.  `DeviceIndex` keeps 128 KiB per VLAD row on the device; a `CompactIndex` keeps m + 4
bytes.  Everything here is float32; the definitions (summation orders, tie rules) are in include/pvsim.h."""
from __future__ import annotations

import numpy as np

from .engine import DeviceBuffer
from .index import DeviceIndex, _PathLedger, _grow_rows, _keep_positions
from .models import PCAModel

__all__ = ["ProductQuantizer", "CompactIndex", "IVFCompactIndex", "fit_projection", "save_arrays", "load_arrays"]

_MAX_PROJECTION_TRAIN = 4096
_CHUNK_ROWS = 8192


def _chunks(n: int):
    """(first row, rows) of the chunks of at most _CHUNK_ROWS rows that n rows go through the device in"""
    for r0 in range(0, n, _CHUNK_ROWS):
        yield r0, min(_CHUNK_ROWS, n - r0)


def _f32_rows(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype == np.float64:
        raise TypeError(f"{what} is float64: the compact index is a float32 structure, pass float32 {what}")
    if a.dtype != np.float32:
        raise TypeError(f"{what} must be float32, got {a.dtype}")
    if a.ndim != 2:
        raise ValueError(f"{what} must be a 2-d array, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _check_rank_args(k, rerank, n: int, kept: bool):
    """-> (k, rerank) as ints, validated against an index of n rows."""
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= n:
        raise ValueError(f"k must be an integer with 1 <= k <= {n} (the number of indexed rows), got {k!r}")
    if isinstance(rerank, bool) or int(rerank) != rerank or rerank < 0:
        raise ValueError(f"rerank must be a non-negative integer, got {rerank!r}")
    k, rerank = int(k), int(rerank)
    if rerank:
        if rerank < k:
            raise ValueError(f"rerank={rerank} must be >= k={k}: the exact re-ranking orders the ADC top-rerank list")
        if not kept:
            raise ValueError("rerank needs the projected rows: build the index with keep_projected=True")
        rerank = min(rerank, n)
    return k, rerank


# ------------------------------------------------------------------------------------------------ projection
def fit_projection(vectors: np.ndarray, n_components: int, ctx=None) -> np.ndarray:
    """W float32 (n_components, L) with orthonormal rows: the top eigenvectors of the UNCENTRED second-moment matrix of the rows.

    No mean is subtracted, deliberately: the projection is there to preserve q.x, and a centred PCA preserves (q - mu).(x - mu),
    a different similarity.  The fit goes by the n x n route (L is 32768 for VLAD, n at most 4096): G = X X^T on the device
    (pvs_cosine_dev with NULL norms), eigh on the host, W = Lambda^(-1/2) U^T X on the device.  More than 4096 training rows are
    subsampled deterministically (evenly spaced).  Rows are sign-fixed as learn.fit_pca does (largest |element| positive)."""
    from .engine import default_context
    from .learn import _one_blas_thread
    x = _f32_rows(vectors, "training vectors")
    n, L = x.shape
    if n > _MAX_PROJECTION_TRAIN:
        x = np.ascontiguousarray(x[(np.arange(_MAX_PROJECTION_TRAIN, dtype=np.int64) * n) // _MAX_PROJECTION_TRAIN])
        n = _MAX_PROJECTION_TRAIN
    d = int(n_components)
    if not 1 <= d <= min(n, L):
        raise ValueError(f"n_components={n_components} must be between 1 and min(n_train, L)={min(n, L)}")
    ctx = ctx or default_context()
    with ctx.scratch() as tmp:
        d_x, d_g = tmp.upload(x), tmp(n * n * 4)
        ctx.cosine_dev(d_x.ptr, n, d_x.ptr, n, L, None, None, d_g.ptr, n)
        g = d_g.download((n, n), np.float32).astype(np.float64)
        g = 0.5 * (g + g.T)
        with _one_blas_thread():
            vals, vecs = np.linalg.eigh(g)
        vals, vecs = vals[::-1][:d], vecs[:, ::-1][:, :d]
        if not vals[-1] > vals[0] * 1e-10:
            raise ValueError(f"the training rows span fewer than n_components={d} dimensions")
        a = np.ascontiguousarray((vecs / np.sqrt(vals)).T, dtype=np.float32)           # Lambda^(-1/2) U^T, (d, n)
        xt = np.ascontiguousarray(x.T)                                                 # (L, n): W = a . (X^T)^T
        d_a, d_xt, d_w = tmp.upload(a), tmp.upload(xt), tmp(d * L * 4)
        ctx.cosine_dev(d_a.ptr, d, d_xt.ptr, L, n, None, None, d_w.ptr, L)
        w = d_w.download((d, L), np.float32)
    piv = np.argmax(np.abs(w), axis=1)
    sign = np.sign(w[np.arange(d), piv])
    sign[sign == 0] = 1
    return np.ascontiguousarray(w * sign[:, None].astype(np.float32))


def _projection_matrix(projection, L: int):
    """None | PCAModel | array -> W float32 (d, L) or None."""
    if projection is None:
        return None
    w = projection.components_ if isinstance(projection, PCAModel) or hasattr(projection, "components_") else projection
    w = np.asarray(w)
    if w.dtype == np.float64:
        raise TypeError("projection is float64: the compact index is a float32 structure, pass a float32 projection")
    w = np.ascontiguousarray(w, dtype=np.float32)
    if w.ndim != 2 or w.shape[1] != L:
        raise ValueError(f"projection must be (d, {L}), got {w.shape}")
    return w


# ------------------------------------------------------------------------------------------------ quantiser
class ProductQuantizer:
    """m sub-spaces of dsub = d / m dimensions, ksub <= 256 codewords each; codes are uint8 (n, m).

    ProductQuantizer(m, ksub).fit(vectors) trains one k-means per sub-space on the device (learn.fit_kmeans);
    ProductQuantizer.from_codebooks(codebooks) takes given tables (m, ksub, dsub)."""

    def __init__(self, m: int, ksub: int = 256, ctx=None):
        if isinstance(m, bool) or int(m) != m or m < 1:
            raise ValueError(f"m must be a positive integer, got {m!r}")
        if isinstance(ksub, bool) or int(ksub) != ksub or not 1 <= ksub <= 256:
            raise ValueError(f"ksub must be between 1 and 256 (codes are one byte per sub-space), got {ksub!r}")
        self.m, self.ksub = int(m), int(ksub)
        self.codebooks = None
        self.projection = None           # optional (d, L) projection that goes with the codebooks (models.save_model kind "pq")
        self._ctx = ctx
        self._table = None

    @classmethod
    def from_codebooks(cls, codebooks, ctx=None) -> "ProductQuantizer":
        c = np.asarray(codebooks)
        if c.dtype == np.float64:
            raise TypeError("codebooks are float64: the compact index is a float32 structure, pass float32 codebooks")
        c = np.ascontiguousarray(c, dtype=np.float32)
        if c.ndim != 3:
            raise ValueError(f"codebooks must be (m, ksub, dsub), got shape {c.shape}")
        pq = cls(c.shape[0], c.shape[1], ctx)
        pq.codebooks = c
        return pq

    @property
    def dsub(self) -> int:
        return 0 if self.codebooks is None else self.codebooks.shape[2]

    @property
    def d(self) -> int:
        return self.m * self.dsub

    @property
    def context(self):
        if self._ctx is None:
            from .engine import default_context
            self._ctx = default_context()
        return self._ctx

    def _check_rows(self, vectors, what="vectors"):
        x = _f32_rows(vectors, what)
        if x.shape[1] % self.m:
            raise ValueError(f"d={x.shape[1]} is not a multiple of m={self.m} (d % m must be 0)")
        return x

    def fit(self, vectors, random_state=None, max_iter: int = 25) -> "ProductQuantizer":
        from .learn import DeviceRows, fit_kmeans, _rng
        x = self._check_rows(vectors, "training vectors")
        n, d = x.shape
        if n < self.ksub:
            raise ValueError(f"n={n} training rows are fewer than ksub={self.ksub} codewords (need n >= ksub)")
        dsub = d // self.m
        rng = _rng(random_state)
        books = np.empty((self.m, self.ksub, dsub), np.float32)
        import warnings
        for s in range(self.m):
            with self.context.scratch() as tmp, warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)             # duplicate points in a sub-space: fewer distinct codewords is fine
                rows = DeviceRows(self.context, n, dsub, tmp.upload(x[:, s * dsub:(s + 1) * dsub]))
                books[s] = fit_kmeans(rows, self.ksub, random_state=rng, max_iter=max_iter).cluster_centers_
        self.codebooks = books
        self._drop_table()
        return self

    def table(self):
        """The device table (engine.PQTable), created on first use."""
        if self.codebooks is None:
            raise ValueError("the quantiser has no codebooks: call fit() or use from_codebooks()")
        if self._table is None or self._table.handle is None:
            self._table = self.context.pq(self.codebooks)
        return self._table

    def _drop_table(self):
        if self._table is not None:
            self._table.close()
            self._table = None

    def encode(self, vectors) -> np.ndarray:
        x = self._check_rows(vectors)
        if self.codebooks is None:
            raise ValueError("the quantiser has no codebooks: call fit() or use from_codebooks()")
        if x.shape[1] != self.d:
            raise ValueError(f"vectors have d={x.shape[1]}, the quantiser d={self.d}")
        n = x.shape[0]
        if n == 0:
            return np.zeros((0, self.m), np.uint8)
        ctx = self.context
        with ctx.scratch() as tmp:
            d_x, d_c = tmp.upload(x), tmp(n * self.m)
            ctx.pq_encode_dev(self.table(), d_x.ptr, n, d_c.ptr)
            return d_c.download((n, self.m), np.uint8)

    def decode(self, codes) -> np.ndarray:
        """codes uint8 (n, m) -> the codewords they name, float32 (n, d)."""
        if self.codebooks is None:
            raise ValueError("the quantiser has no codebooks: call fit() or use from_codebooks()")
        c = np.asarray(codes)
        if c.ndim != 2 or c.shape[1] != self.m:
            raise ValueError(f"codes must be (n, {self.m}), got {c.shape}")
        if c.size and int(c.max()) >= self.ksub:
            raise ValueError(f"a code exceeds ksub={self.ksub}")
        return np.concatenate([self.codebooks[s][c[:, s].astype(np.int64)] for s in range(self.m)], axis=1)

    def close(self):
        self._drop_table()


# ------------------------------------------------------------------------------------------------ persistence (no device needed)
_KINDS = {"compact_index": "compact index", "ivf_compact_index": "IVF compact index"}


def save_arrays(path: str, paths, codes, inv_norms, codebooks, projection=None, projected=None, kind: str = "compact_index",
                **more) -> None:
    """One plain .npz of arrays (numpy.load(allow_pickle=False)), in the style of pvsim.index.  `more`: further arrays of the kind
    (an IVF index adds centroids, list_off and ids)."""
    arrays = dict(kind=kind, paths=np.array(list(paths), dtype=np.str_), codes=np.ascontiguousarray(codes, dtype=np.uint8),
                  inv_norms=np.ascontiguousarray(inv_norms, dtype=np.float32), codebooks=np.ascontiguousarray(codebooks, dtype=np.float32))
    if projection is not None:
        arrays["projection"] = np.ascontiguousarray(projection, dtype=np.float32)
    if projected is not None:
        arrays["projected"] = np.ascontiguousarray(projected, dtype=np.float32)
    arrays.update(more)
    np.savez(path, **arrays)


def load_arrays(path: str, kind: str = "compact_index", more=()) -> dict:
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
        if "kind" not in z.files or str(z["kind"]) != kind:
            raise ValueError(f"{path}: not a{'n' if kind[0] in 'aeiou' else ''} {_KINDS[kind]} file")
        out = dict(paths=[str(p) for p in z["paths"]], codes=z["codes"], inv_norms=z["inv_norms"], codebooks=z["codebooks"],
                   projection=z["projection"] if "projection" in z.files else None,
                   projected=z["projected"] if "projected" in z.files else None)
        out.update({name: z[name] for name in more})
    return out


# ------------------------------------------------------------------------------------------------ index
class CompactIndex:
    """Paths + uint8 codes (N, m) + float32 1/||row|| (N,) resident on the device, searched by pvs_pq_scan_topk_dev.

    `projection` is None (d = L), a PCAModel (its components_ are used; no mean is subtracted) or an array (d, L);
    `projected` are the projected float32 rows (N, d), kept only for exact re-ranking (`rank(..., rerank=R)`).
    The arrays are uploaded on first use.  `add` and `remove` change the resident index without a rebuild:
    new rows go through the entry points `fit` uses, rows move on the device, nothing is retrained, and every array and ranking
    equals those of an index constructed from the surviving rows in surviving order with the same tables."""

    def __init__(self, paths, codes, inv_norms, quantizer, projection=None, projected=None, ctx=None):
        if not isinstance(quantizer, ProductQuantizer):
            quantizer = ProductQuantizer.from_codebooks(quantizer, ctx)
        if quantizer.codebooks is None:
            raise ValueError("the quantiser has no codebooks")
        self.quantizer = quantizer
        self._paths = [str(p) for p in paths]
        n = len(self._paths)
        codes = np.asarray(codes)
        if codes.dtype != np.uint8 or codes.shape != (n, quantizer.m):
            raise ValueError(f"codes must be uint8 ({n}, {quantizer.m}), got {codes.dtype} {codes.shape}")
        inv = np.asarray(inv_norms)
        if inv.dtype == np.float64:
            raise TypeError("inv_norms are float64: the compact index is a float32 structure, pass float32 inv_norms")
        if inv.shape != (n,):
            raise ValueError(f"inv_norms must be ({n},), got {inv.shape}")
        self._L = None if projection is None else int(np.asarray(getattr(projection, "components_", projection)).shape[1])
        self._w = _projection_matrix(projection, self._L) if projection is not None else None
        if self._w is not None and self._w.shape[0] != quantizer.d:
            raise ValueError(f"the projection gives d={self._w.shape[0]}, the quantiser has d={quantizer.d}")
        self._keep = projected is not None
        if self._keep:
            projected = _f32_rows(projected, "projected rows")
            if projected.shape != (n, quantizer.d):
                raise ValueError(f"projected rows must be ({n}, {quantizer.d}), got {projected.shape}")
        self._ctx = ctx or quantizer._ctx
        self._host = dict(codes=np.ascontiguousarray(codes), inv=np.ascontiguousarray(inv, dtype=np.float32), projected=projected)
        self._dev = None

    # ---- building
    @classmethod
    def fit(cls, source, m: int = 64, n_components=None, projection=None, ksub: int = 256, keep_projected: bool = False,
            random_state=None, train=None, ctx=None, max_iter: int = 25) -> "CompactIndex":
        """Train the projection and the quantiser on `train` (default: the database itself), project the database, record
        1/||projected row||, encode, and keep codes, norms and paths on the device.  `source` is an encoding map {path: vector}
        or a DeviceIndex (whose resident rows are read in place)."""
        return cls._fit(source, m, n_components, projection, ksub, keep_projected, random_state, train, ctx, max_iter)

    @classmethod
    def _fit(cls, source, m, n_components, projection, ksub, keep_projected, random_state, train, ctx, max_iter, nlist=None):
        """fit(); with `nlist` the rows are assigned to nlist coarse centroids (k-means on the projected training rows) and the
        quantiser is trained on, and encodes, their residuals (IVFCompactIndex)."""
        from .engine import default_context
        resident = source if isinstance(source, DeviceIndex) else None
        if resident is not None:
            paths, mat = list(resident.keys()), resident.matrix
            ctx = ctx or resident.ctx
        else:
            paths = list(source.keys())
            mat = np.array(list(source.values()))
        mat = _f32_rows(mat, "database")
        n, L = mat.shape
        if n_components is not None and projection is not None:
            raise ValueError("give n_components or projection, not both")
        pq = ProductQuantizer(m, ksub, ctx)                                  # validates m, ksub before anything is computed
        tr = mat if train is None else _f32_rows(np.array(list(train.values())) if hasattr(train, "values") else train, "train")
        if tr.shape[1] != L:
            raise ValueError(f"train rows have L={tr.shape[1]}, the database L={L}")
        d = L if (n_components is None and projection is None) else (
            int(n_components) if n_components is not None else int(np.asarray(getattr(projection, "components_", projection)).shape[0]))
        if d % pq.m:
            raise ValueError(f"d={d} is not a multiple of m={pq.m} (d % m must be 0)")
        if tr.shape[0] < pq.ksub:
            raise ValueError(f"n={tr.shape[0]} training rows are fewer than ksub={pq.ksub} codewords (need n >= ksub)")
        if nlist is not None:
            nlist = _check_nlist(nlist, tr.shape[0], n)
        ctx = ctx or default_context()
        pq._ctx = ctx
        w = fit_projection(tr, n_components, ctx) if n_components is not None else _projection_matrix(projection, L)

        def projected(chunk, host, r0, rn, dev_ptr=None, dest=None):
            """rows [r0, r0 + rn) of the matrix, projected -> device buffer (rn, d): `dest(r0, rn)` (a view into the kept rows, not
            owned) or a temporary of the scratch scope `chunk`"""
            out = dest(r0, rn) if dest is not None else chunk(rn * d * 4)
            if d_w is None:                          # no projection: the rows themselves
                out.upload(host[r0:r0 + rn])
            elif dev_ptr is not None:                # resident rows are read in place
                ctx.cosine_dev(dev_ptr + r0 * L * 4, rn, d_w.ptr, d, L, None, None, out.ptr, d)
            else:
                with ctx.scratch() as own:
                    ctx.cosine_dev(own.upload(host[r0:r0 + rn]).ptr, rn, d_w.ptr, d, L, None, None, out.ptr, d)
                    ctx.sync()
            return out

        try:
            with ctx.scratch() as tmp:               # device buffers of this call; what the index keeps leaves the scope at the end
                d_w = tmp.upload(w) if w is not None else None
                db_ptr = resident._db.ptr if resident is not None else None
                # the quantiser is trained on the projected training rows
                ytr = np.empty((tr.shape[0], d), np.float32)
                for r0, rn in _chunks(tr.shape[0]):
                    with ctx.scratch() as chunk:
                        ytr[r0:r0 + rn] = projected(chunk, tr, r0, rn, db_ptr if train is None else None).download((rn, d), np.float32)
                d_cent = d_lists = d_res = None
                if nlist is None:
                    pq.fit(ytr, random_state=random_state, max_iter=max_iter)
                else:                                    # coarse centroids, then the quantiser on the training rows' residuals
                    from .learn import _rng
                    rng = _rng(random_state)
                    cent = _fit_coarse(ctx, ytr, nlist, rng, max_iter)
                    d_cent = tmp.upload(cent)
                    res = np.empty_like(ytr)
                    for r0, rn in _chunks(ytr.shape[0]):
                        with ctx.scratch() as chunk:
                            d_y, d_l, d_r = chunk.upload(ytr[r0:r0 + rn]), chunk(rn * 4), chunk(rn * d * 4)
                            ctx.ivf_assign_dev(d_y.ptr, rn, d, d_cent.ptr, nlist, d_l.ptr, d_r.ptr)
                            res[r0:r0 + rn] = d_r.download((rn, d), np.float32)
                    pq.fit(res, random_state=rng, max_iter=max_iter)
                    del res
                    d_lists, d_res = tmp(n * 4), tmp(min(n, _CHUNK_ROWS) * d * 4)
                table = pq.table()
                # the arrays `add` appends to hold at least 16 bytes: _reserve_rows reads their size as the capacity
                d_codes, d_inv = tmp(max(n * pq.m, 16)), tmp(max(n * 4, 16))
                d_proj = tmp(max(n * d * 4, 16)) if keep_projected else None
                # kept rows are written where they stay: a chunk's buffer is then a view into d_proj
                dest = (lambda r0, rn: DeviceBuffer.view(ctx, d_proj.ptr + r0 * d * 4, rn * d * 4)) if keep_projected else None
                for r0, rn in _chunks(n):
                    with ctx.scratch() as chunk:
                        if train is None:                # the database was the training set: its projected rows are in ytr
                            buf = (dest(r0, rn) if dest is not None else chunk(rn * d * 4)).upload(ytr[r0:r0 + rn])
                        else:
                            buf = projected(chunk, mat, r0, rn, db_ptr, dest)
                        ctx.row_inv_norms_dev(buf.ptr, rn, d, d_inv.ptr + r0 * 4)
                        if nlist is None:
                            ctx.pq_encode_dev(table, buf.ptr, rn, d_codes.ptr + r0 * pq.m)
                        else:
                            ctx.ivf_assign_dev(buf.ptr, rn, d, d_cent.ptr, nlist, d_lists.ptr + r0 * 4, d_res.ptr)
                            ctx.pq_encode_dev(table, d_res.ptr, rn, d_codes.ptr + r0 * pq.m)
                        ctx.sync()
                dev = dict(codes=d_codes, inv=d_inv, projected=d_proj, w=None)
                if nlist is not None:                    # sort into lists: by (list, original index), on the host
                    ids, list_off = _sort_into_lists(d_lists.download((n,), np.int32), nlist)
                    d_codes.upload(np.ascontiguousarray(d_codes.download((n, pq.m), np.uint8)[ids]))
                    d_inv.upload(np.ascontiguousarray(d_inv.download((n,), np.float32)[ids]))
                    dev.update(cent=d_cent, ids=tmp.upload(ids), list_off=tmp.upload(list_off))
                for b in dev.values():                   # these are the index's from here on
                    tmp.keep(b)
        except BaseException:
            pq.close()                               # the quantiser's device table
            raise
        self = cls.__new__(cls)
        self.quantizer, self._paths, self._ctx = pq, [str(p) for p in paths], ctx
        self._L, self._w, self._keep, self._host = L, w, bool(keep_projected), None
        self._dev = dev
        if nlist is not None:
            self._centroids, self._list_off, self._ids = cent, list_off, ids
        return self

    # ---- device residency
    @property
    def context(self):
        if self._ctx is None:
            from .engine import default_context
            self._ctx = default_context()
        return self._ctx

    def _device(self) -> dict:
        if self._dev is None:
            ctx, h = self.context, self._host
            self._dev = dict(codes=ctx.buffer(max(h["codes"].nbytes, 16)).upload(h["codes"]),
                             inv=ctx.buffer(max(h["inv"].nbytes, 16)).upload(h["inv"]),
                             projected=ctx.buffer(max(h["projected"].nbytes, 16)).upload(h["projected"]) if self._keep else None,
                             w=None)
            self._host = None
        if self._w is not None and self._dev["w"] is None:
            self._dev["w"] = self.context.buffer(self._w.nbytes).upload(self._w)
        return self._dev

    # ---- the dict-like surface the retrieval functions use
    @property
    def _paths(self) -> list:
        """the paths in index order: the ledger's own list, not a copy"""
        return self._ledger.paths

    @_paths.setter
    def _paths(self, paths):
        self._ledger = _PathLedger(paths)

    def __len__(self):
        return len(self._ledger)

    @property
    def paths(self) -> list:
        return list(self._paths)

    def keys(self):
        return list(self._paths)

    @property
    def d(self) -> int:
        return self.quantizer.d

    @property
    def input_dim(self) -> int:
        """length of the vectors `rank` takes (L with a projection, d without)"""
        return self._w.shape[1] if self._w is not None else self.quantizer.d

    @property
    def projection(self):
        return self._w

    @property
    def nbytes_breakdown(self) -> dict:
        n, q = len(self), self.quantizer
        return {"codes": n * q.m, "inv_norms": n * 4, "codebooks": q.m * q.ksub * q.dsub * 4,
                "projection": 0 if self._w is None else self._w.nbytes, "projected": n * q.d * 4 if self._keep else 0}

    @property
    def nbytes(self) -> int:
        """device bytes: N (m + 4) for codes and norms, plus the tables (and the projected rows when they are kept)"""
        return int(sum(self.nbytes_breakdown.values()))

    def _download(self):
        n, q, dev = len(self), self.quantizer, self._device()
        return (dev["codes"].download((n, q.m), np.uint8), dev["inv"].download((n,), np.float32),
                dev["projected"].download((n, q.d), np.float32) if self._keep else None)

    def project(self, vectors) -> np.ndarray:
        """The device's own projection of float32 rows (n, input_dim) -> (n, d)."""
        x = _f32_rows(vectors, "vectors")
        if x.shape[1] != self.input_dim:
            raise ValueError(f"vectors have {x.shape[1]} dimensions, the index takes {self.input_dim}")
        if self._w is None or x.shape[0] == 0:
            return x.copy() if self._w is None else np.zeros((0, self.d), np.float32)
        ctx, dev = self.context, self._device()
        with ctx.scratch() as tmp:
            d_x, d_y = tmp.upload(x), tmp(x.shape[0] * self.d * 4)
            ctx.cosine_dev(d_x.ptr, x.shape[0], dev["w"].ptr, self.d, x.shape[1], None, None, d_y.ptr, self.d)
            return d_y.download((x.shape[0], self.d), np.float32)

    # ---- updates
    def _check_new(self, source):
        """-> (paths, float32 host rows (b, input_dim), the DeviceIndex they are resident in or None); touches no device"""
        resident = source if isinstance(source, DeviceIndex) else None
        paths = [str(p) for p in source.keys()]
        if resident is not None:
            mat = resident.matrix
        else:
            mat = np.array(list(source.values())) if paths else np.zeros((0, self.input_dim), np.float32)
        mat = _f32_rows(mat, "new vectors")
        if mat.shape[1] != self.input_dim:
            raise ValueError(f"new vectors have {mat.shape[1]} dimensions, the index takes {self.input_dim}")
        self._ledger.check_new(paths)
        self._check_size(len(self) + len(paths))
        return paths, mat, resident

    def _check_size(self, n: int) -> None:
        pass

    def _reserve_rows(self, dev: dict, name: str, row_bytes: int, used: int, need: int) -> None:
        """room for `need` rows in dev[name], growing geometrically; the first `used` rows are copied on the device"""
        have = dev[name].nbytes // row_bytes
        if have < need:
            dev[name] = _grow_rows(self.context, dev[name], row_bytes, used, max(need, 2 * have))

    def reserve(self, n: int) -> None:
        """Room for n rows in the device buffers an `add` appends to (codes and norms of a flat index, the kept projected rows)."""
        dev, used = self._device(), len(self)
        for name, row_bytes in self._appended(dev):
            self._reserve_rows(dev, name, row_bytes, used, int(n))

    def _appended(self, dev: dict):
        """(buffer name, bytes per row) of the arrays that grow by appending"""
        q = self.quantizer
        return [("codes", q.m), ("inv", 4)] + ([("projected", q.d * 4)] if self._keep else [])

    def _encode_new(self, mat, resident, d_codes: int, d_inv: int, d_proj, d_lists, tmp):
        """The b new rows through project -> row_inv_norms_dev -> (ivf_assign_dev + residual) -> pq_encode_dev, in chunks: codes
        to d_codes, norms to d_inv, the projected rows to d_proj (or nowhere), list numbers to d_lists (an IVF index).  Raw device
        addresses; the temporaries belong to the caller's scratch scope `tmp` and live until it ends."""
        ctx, dev, pq = self.context, self._device(), self.quantizer
        d, m, L, table = pq.d, pq.m, self.input_dim, pq.table()
        d_res = tmp(min(mat.shape[0], _CHUNK_ROWS) * d * 4) if d_lists is not None else None
        for r0, rn in _chunks(mat.shape[0]):
            src = resident._db.ptr + r0 * L * 4 if resident is not None else tmp.upload(mat[r0:r0 + rn]).ptr
            if self._w is None and d_proj is None:
                y = src                                            # no projection: the rows themselves, where they are
            else:
                y = d_proj + r0 * d * 4 if d_proj is not None else tmp(rn * d * 4).ptr
                if self._w is None:
                    ctx.copy_dev(y, src, rn * d * 4)
                else:
                    ctx.cosine_dev(src, rn, dev["w"].ptr, d, L, None, None, y, d)
            ctx.row_inv_norms_dev(y, rn, d, d_inv + r0 * 4)
            if d_lists is None:
                ctx.pq_encode_dev(table, y, rn, d_codes + r0 * m)
            else:
                ctx.ivf_assign_dev(y, rn, d, dev["cent"].ptr, self.nlist, d_lists + r0 * 4, d_res.ptr)
                ctx.pq_encode_dev(table, d_res.ptr, rn, d_codes + r0 * m)

    def add(self, source) -> None:
        """Append new images: `source` is {path: vector of input_dim} or a DeviceIndex whose resident rows are read in place.  They
        get the original indices N, N + 1, ... in the order given.  A path that is already indexed is a ValueError, raised before
        anything changes.  The projection, the codebooks (and the coarse centroids) stay as they are."""
        paths, mat, resident = self._check_new(source)
        if not paths:
            return
        dev, n, b = self._device(), len(self), len(paths)
        with self.context.scratch() as tmp:
            for name, row_bytes in self._appended(dev):
                self._reserve_rows(dev, name, row_bytes, n, n + b)
            self._append(dev, mat, resident, n, tmp)
        self._ledger.append(paths)
        self._drop_caches(dev)

    def _append(self, dev, mat, resident, n, tmp) -> None:
        q = self.quantizer
        self._encode_new(mat, resident, dev["codes"].ptr + n * q.m, dev["inv"].ptr + n * 4,
                         dev["projected"].ptr + n * q.d * 4 if self._keep else None, None, tmp)

    def remove(self, paths) -> None:
        """The named images leave, the others keep their relative order; the original index of a survivor falls by the number of
        removed rows before it.  An unknown path is a KeyError, a path named twice a ValueError, both raised before anything changes."""
        idx = self._ledger.removed_indices([paths] if isinstance(paths, str) else [str(p) for p in paths])
        if idx.size == 0:
            return
        ctx, dev, n = self.context, self._device(), len(self)
        with ctx.scratch() as tmp:
            keep, pos = _keep_positions(tmp, idx, n)
            self._remove_stored(tmp, dev, n, idx, keep, pos)
            if self._keep:
                ctx.compact_rows_dev(dev["projected"].ptr, n, self.quantizer.d * 4, keep.ptr, pos.ptr, dev["projected"].ptr, first=int(idx[0]))
        self._ledger.remove(idx)
        self._drop_caches(dev)

    def __delitem__(self, path) -> None:
        self.remove([path])

    def _remove_stored(self, tmp, dev, n, idx, keep, pos) -> None:
        for name, row_bytes in (("codes", self.quantizer.m), ("inv", 4)):
            tmp.ctx.compact_rows_dev(dev[name].ptr, n, row_bytes, keep.ptr, pos.ptr, dev[name].ptr, first=int(idx[0]))

    def _drop_caches(self, dev) -> None:
        """what was derived from the arrays an update has changed"""

    # ---- search
    def rank(self, query_vecs, k: int, rerank: int = 0):
        """-> (idx (nq, k) int64, val (nq, k) float32): the ADC ranking (score descending, index ascending); with rerank=R >= k
        the ADC top-R re-scored exactly against the kept projected rows and ordered by (exact score descending, index ascending)."""
        return self._rank(query_vecs, k, rerank)

    def _scan(self, ctx, dev, tmp, d_y, d_invq, d_lut, nq, kk, d_idx, d_val):
        """the ADC lists of nq projected queries (rows d_y, tables d_lut) into d_idx / d_val (nq, kk); `tmp`: the caller's scratch scope"""
        n, pq = len(self), self.quantizer
        ctx.pq_scan_topk_dev(d_lut.ptr, nq, pq.m, pq.ksub, dev["codes"].ptr, n, d_invq.ptr, dev["inv"].ptr, kk, 0, False,
                             d_idx.ptr, d_val.ptr)

    def _check_rank_args(self, k, rerank):
        return _check_rank_args(k, rerank, len(self), self._keep)

    def _rescore_norms(self, dev):
        """1/||row|| indexed like the kept projected rows (by original index)"""
        return dev["inv"]

    def _rank(self, query_vecs, k, rerank, **scan_args):
        q = _f32_rows(query_vecs, "query")
        if q.shape[1] != self.input_dim:
            raise ValueError(f"query and database dimensions differ: {q.shape[1]} vs {self.input_dim}")
        n, pq = len(self), self.quantizer
        k, rerank = self._check_rank_args(k, rerank, **scan_args)
        nq, d, kk = q.shape[0], pq.d, rerank or k
        if nq == 0:
            return np.zeros((0, k), np.int64), np.zeros((0, k), np.float32)
        ctx, dev = self.context, self._device()
        with ctx.scratch() as tmp:
            d_q = tmp.upload(q)
            if self._w is not None:
                d_y = tmp(nq * d * 4)
                ctx.cosine_dev(d_q.ptr, nq, dev["w"].ptr, d, q.shape[1], None, None, d_y.ptr, d)
            else:
                d_y = d_q
            d_invq, d_lut = tmp(nq * 4), tmp(nq * pq.m * pq.ksub * 4)
            d_idx, d_val = tmp(nq * kk * 8), tmp(nq * kk * 4)
            ctx.row_inv_norms_dev(d_y.ptr, nq, d, d_invq.ptr)
            ctx.pq_lut_dev(pq.table(), d_y.ptr, nq, d_lut.ptr)
            self._scan(ctx, dev, tmp, d_y, d_invq, d_lut, nq, kk, d_idx, d_val, **scan_args)
            if not rerank:
                return d_idx.download((nq, k), np.int64), d_val.download((nq, k), np.float32)
            d_exact = tmp(nq * kk * 4)
            ctx.rescore_rows_dev(d_y.ptr, nq, dev["projected"].ptr, n, d, d_invq.ptr, self._rescore_norms(dev).ptr, d_idx.ptr, kk,
                                 d_exact.ptr)
            idx, val = d_idx.download((nq, kk), np.int64), d_exact.download((nq, kk), np.float32)
        return order_exact(idx, val, k)

    # ---- persistence
    def save(self, path: str) -> None:
        codes, inv, proj = self._download()
        save_arrays(path, self._paths, codes, inv, self.quantizer.codebooks, self._w, proj)

    @classmethod
    def load(cls, path: str, ctx=None) -> "CompactIndex":
        a = load_arrays(path)
        return cls(a["paths"], a["codes"], a["inv_norms"], ProductQuantizer.from_codebooks(a["codebooks"], ctx), a["projection"],
                   a["projected"], ctx)

    def close(self):
        if self._dev is not None:
            for b in self._dev.values():
                if b is not None:
                    b.free()
            self._dev = None
        self.quantizer.close()


def order_exact(idx: np.ndarray, val: np.ndarray, k: int):
    """Rows of candidates -> the first k by (score descending, index ascending), NaN last."""
    out_i = np.empty((idx.shape[0], k), np.int64)
    out_v = np.empty((idx.shape[0], k), np.float32)
    for r in range(idx.shape[0]):
        nan = np.isnan(val[r])
        key = np.where(nan, np.float32(-np.inf), val[r])
        o = np.lexsort((idx[r], -key, nan))[:k]
        out_i[r], out_v[r] = idx[r][o], val[r][o]
    return out_i, out_v


# ------------------------------------------------------------------------------------------------ inverted lists
MAX_NPROBE = 1024
MAX_IVF_K = 1024
MAX_NLIST = 65536


def _check_nlist(nlist, n_train: int, n: int) -> int:
    if isinstance(nlist, bool) or int(nlist) != nlist or not 1 <= nlist <= MAX_NLIST:
        raise ValueError(f"nlist must be an integer between 1 and {MAX_NLIST}, got {nlist!r}")
    if n_train < nlist:
        raise ValueError(f"n={n_train} training rows are fewer than nlist={nlist} coarse centroids (need n >= nlist)")
    if n >= 2 ** 31:
        raise ValueError(f"an IVF compact index holds fewer than 2^31 rows, got {n}")
    return int(nlist)


def _fit_coarse(ctx, rows: np.ndarray, nlist: int, rng, max_iter: int) -> np.ndarray:
    """coarse centroids float32 (nlist, d): learn.fit_kmeans on the projected training rows"""
    import warnings
    from .learn import DeviceRows, fit_kmeans
    with ctx.scratch() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                 # duplicate rows: fewer distinct centroids, some lists stay empty
        dev = DeviceRows(ctx, *rows.shape, tmp.upload(rows))
        return np.ascontiguousarray(fit_kmeans(dev, nlist, random_state=rng, max_iter=max_iter).cluster_centers_, dtype=np.float32)


def _sort_into_lists(lists: np.ndarray, nlist: int):
    """list of every row -> (ids int32 (N,): the original index of each stored row, rows sorted by (list, original index);
    list_off int64 (nlist + 1,))"""
    lists = np.asarray(lists)
    if lists.size and (int(lists.min()) < 0 or int(lists.max()) >= nlist):
        raise ValueError(f"a list number lies outside [0, {nlist})")
    ids = np.argsort(lists, kind="stable").astype(np.int32)
    list_off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(lists, minlength=nlist), out=list_off[1:])
    return ids, list_off


class IVFCompactIndex(CompactIndex):
    """A CompactIndex cut into `nlist` inverted lists (IVFADC; Jegou, Douze, Schmid, PAMI 2011): coarse centroids (nlist, d), the rows
    stored sorted by (list, original index) and product-quantised as residuals to their list's centroid.  `rank` scans the
    `nprobe` lists whose centroids score best against the query: about nprobe / nlist of the rows.

    `codes` and `inv_norms` are in STORED order, `ids` (N,) int32 names the original index of each stored row (the index into
    `paths`, and into `projected`, which stays in original order), `list_off` (nlist + 1,) int64 bounds the lists."""

    def __init__(self, paths, codes, inv_norms, quantizer, centroids, list_off, ids, projection=None, projected=None, ctx=None):
        super().__init__(paths, codes, inv_norms, quantizer, projection, projected, ctx)
        n = len(self._paths)
        cent = np.asarray(centroids)
        if cent.dtype == np.float64:
            raise TypeError("centroids are float64: the compact index is a float32 structure, pass float32 centroids")
        if cent.dtype != np.float32 or cent.ndim != 2 or cent.shape[1] != self.quantizer.d or not 1 <= cent.shape[0] <= MAX_NLIST:
            raise ValueError(f"centroids must be float32 (nlist, {self.quantizer.d}) with 1 <= nlist <= {MAX_NLIST}, got {cent.dtype} "
                             f"{cent.shape}")
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
            raise ValueError(f"an IVF compact index holds fewer than 2^31 rows, got {n}")
        if n and not np.array_equal(np.sort(ids), np.arange(n)):
            raise ValueError(f"ids must be a permutation of 0 .. {n - 1}")
        self._centroids, self._list_off, self._ids = np.ascontiguousarray(cent), off, np.ascontiguousarray(ids, dtype=np.int32)

    @property
    def _ids(self) -> np.ndarray:
        """host copy of the stored rows' original indices: downloaded when `save`, a property or a check needs it after an update"""
        if self._ids_host is None:
            n = len(self)
            self._ids_host = self._dev["ids"].download((n,), np.int32) if n else np.zeros(0, np.int32)
        return self._ids_host

    @_ids.setter
    def _ids(self, ids):
        self._ids_host = ids

    @classmethod
    def fit(cls, source, nlist: int, m: int = 64, n_components=None, projection=None, ksub: int = 256, keep_projected: bool = False,
            random_state=None, train=None, ctx=None, max_iter: int = 25) -> "IVFCompactIndex":
        """CompactIndex.fit with a coarse quantiser: project, train `nlist` coarse centroids on the projected training rows
        (learn.fit_kmeans), assign the rows, train the product quantiser on the training rows' residuals, encode the residuals,
        sort the rows into their lists, and keep everything on the device."""
        _check_nlist(nlist, nlist, 0)                # the type and range, before anything is computed
        return cls._fit(source, m, n_components, projection, ksub, keep_projected, random_state, train, ctx, max_iter, nlist=nlist)

    # ---- device residency
    def _device(self) -> dict:
        fresh = self._dev is None
        dev = super()._device()
        if fresh:
            ctx = self.context
            for name, a in (("cent", self._centroids), ("ids", self._ids), ("list_off", self._list_off)):
                dev[name] = ctx.buffer(a.nbytes).upload(a)
        return dev

    @property
    def nlist(self) -> int:
        return self._centroids.shape[0]

    @property
    def centroids(self) -> np.ndarray:
        return self._centroids

    @property
    def list_sizes(self) -> np.ndarray:
        """rows per inverted list, int64 (nlist,)"""
        return np.diff(self._list_off)

    @property
    def nbytes_breakdown(self) -> dict:
        out = super().nbytes_breakdown
        out.update(centroids=self._centroids.nbytes, ids=len(self) * 4, list_off=self._list_off.nbytes,
                   inv_norms_original=len(self) * 4 if self._keep else 0)
        return out

    def _rescore_norms(self, dev):
        """the stored norms are in list order, the kept rows in original order: exact re-scoring reads a copy of the norms in
        original order (4 bytes per row, only beside kept rows; made on the first re-ranking)"""
        if dev.get("inv_orig") is None:
            stored = dev["inv"].download((len(self),), np.float32)
            orig = np.empty_like(stored)
            orig[self._ids] = stored
            dev["inv_orig"] = self.context.buffer(orig.nbytes).upload(orig)
        return dev["inv_orig"]

    # ---- updates
    def _check_size(self, n: int) -> None:
        if n >= 2 ** 31:
            raise ValueError(f"an IVF compact index holds fewer than 2^31 rows, got {n}")

    def _appended(self, dev: dict):
        """the stored arrays are merged into fresh buffers by every insert; only the kept rows grow by appending"""
        return [("projected", self.quantizer.d * 4)] if self._keep else []

    def _swap_stored(self, dev, codes, inv, ids, off, list_off) -> None:
        for name, new in (("codes", codes), ("inv", inv), ("ids", ids), ("list_off", off)):
            dev[name].free()
            dev[name] = new
        self._list_off, self._ids_host = list_off, None

    def _append(self, dev, mat, resident, n, tmp) -> None:
        """encode the new rows, sort their list numbers on the host (b entries), merge old and new storage on the device"""
        q, nlist, b = self.quantizer, self.nlist, mat.shape[0]
        d_codes, d_inv, d_lists = tmp(b * q.m), tmp(b * 4), tmp(b * 4)
        self._encode_new(mat, resident, d_codes.ptr, d_inv.ptr, dev["projected"].ptr + n * q.d * 4 if self._keep else None, d_lists.ptr,
                         tmp)
        perm, new_off = _sort_into_lists(d_lists.download((b,), np.int32), nlist)
        d_perm, d_new_off = tmp.upload(perm), tmp.upload(new_off)
        out = [tmp(nbytes) for nbytes in ((n + b) * q.m, (n + b) * 4, (n + b) * 4, (nlist + 1) * 8)]
        tmp.ctx.ivf_insert_dev(q.m, nlist, dev["codes"].ptr, dev["inv"].ptr, dev["ids"].ptr, dev["list_off"].ptr, self._list_off,
                               d_codes.ptr, d_inv.ptr, d_new_off.ptr, new_off, d_perm.ptr, *(o.ptr for o in out))
        self._swap_stored(dev, *(tmp.keep(o) for o in out), self._list_off + new_off)

    def _remove_stored(self, tmp, dev, n, idx, keep, pos) -> None:
        q, nlist, left = self.quantizer, self.nlist, n - idx.size
        out = [tmp(nbytes) for nbytes in (left * q.m, left * 4, left * 4, (nlist + 1) * 8)]
        tmp.ctx.ivf_remove_dev(q.m, nlist, n, dev["codes"].ptr, dev["inv"].ptr, dev["ids"].ptr, dev["list_off"].ptr, keep.ptr, pos.ptr,
                               *(o.ptr for o in out))
        list_off = out[3].download((nlist + 1,), np.int64)
        self._swap_stored(dev, *(tmp.keep(o) for o in out), list_off)

    def _drop_caches(self, dev) -> None:
        if dev.get("inv_orig") is not None:                # the norms in original order: remade on the next re-ranking
            dev["inv_orig"].free()
            dev["inv_orig"] = None

    # ---- search
    def rank(self, query_vecs, k: int, nprobe: int, rerank: int = 0):
        """-> (idx (nq, k) int64, val (nq, k) float32): the ADC ranking over the `nprobe` best lists of each query, by (score
        descending, original index ascending); slots the probed lists cannot fill are -1 / -inf.  rerank=R >= k re-scores the
        ADC top-R exactly against the kept projected rows; unfilled slots stay last."""
        return self._rank(query_vecs, k, rerank, nprobe=nprobe)

    def _check_rank_args(self, k, rerank, nprobe):
        if isinstance(nprobe, bool) or nprobe is None or int(nprobe) != nprobe or not 1 <= nprobe <= min(self.nlist, MAX_NPROBE):
            raise ValueError(f"nprobe must be an integer with 1 <= nprobe <= {min(self.nlist, MAX_NPROBE)} (min(nlist, {MAX_NPROBE})), "
                             f"got {nprobe!r}")
        k, rerank = _check_rank_args(k, rerank, len(self), self._keep)
        if max(k, rerank) > MAX_IVF_K:
            raise ValueError(f"an IVFCompactIndex ranks at most {MAX_IVF_K} entries per query (k and rerank), got k={k}, rerank={rerank}")
        return k, rerank

    def _scan(self, ctx, dev, tmp, d_y, d_invq, d_lut, nq, kk, d_idx, d_val, nprobe):
        pq, nlist, nprobe = self.quantizer, self.nlist, int(nprobe)
        d_coarse, d_pidx, d_pval = tmp(nq * nlist * 4), tmp(nq * nprobe * 8), tmp(nq * nprobe * 4)
        ctx.ivf_coarse_dev(d_y.ptr, nq, pq.d, dev["cent"].ptr, nlist, d_coarse.ptr)
        ctx.topk_dev(d_coarse.ptr, nq, nlist, nlist, nprobe, 0, False, d_pidx.ptr, d_pval.ptr)
        ctx.ivf_scan_topk_dev(d_lut.ptr, nq, pq.m, pq.ksub, d_pidx.ptr, d_pval.ptr, nprobe, dev["list_off"].ptr, self._list_off, nlist,
                              dev["codes"].ptr, dev["ids"].ptr, d_invq.ptr, dev["inv"].ptr, kk, d_idx.ptr, d_val.ptr)

    # ---- persistence
    def save(self, path: str) -> None:
        codes, inv, proj = self._download()
        save_arrays(path, self._paths, codes, inv, self.quantizer.codebooks, self._w, proj, kind="ivf_compact_index",
                    centroids=self._centroids, list_off=self._list_off, ids=self._ids)

    @classmethod
    def load(cls, path: str, ctx=None) -> "IVFCompactIndex":
        a = load_arrays(path, kind="ivf_compact_index", more=("centroids", "list_off", "ids"))
        return cls(a["paths"], a["codes"], a["inv_norms"], ProductQuantizer.from_codebooks(a["codebooks"], ctx), a["centroids"],
                   a["list_off"], a["ids"], a["projection"], a["projected"], ctx)
