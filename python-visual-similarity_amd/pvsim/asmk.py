"""Local-descriptor retrieval: an ASMK* index with binary signatures on the MI355X.

The aggregated selective match kernel in its binary form (Tolias, Avrithis, Jegou, "To aggregate or not to aggregate", ICCV 2013,
on Jegou's Hamming embedding): a large vocabulary; per image and visual word the summed residual of the rows assigned to the word,
reduced to a B-bit signature; an inverted file over words; a score that sums a selectivity function of the Hamming distance over
the words two images share.  It searches a database by the local descriptors themselves, and is the first stage for
`eval.rerank_spatial` on the same `LocalFeatureIndex`:

    local = LocalFeatureIndex.from_images(paths)
    index = ASMKIndex.fit(local, n_words=65536)                  # or ASMKIndex.build(local, vocabulary)
    hits = index.retrieve(query_image, k=100)                    # [(path, score)]; ma=5 assigns every query row to its 5 nearest words
    ranked = eval.rerank_spatial(query_image, hits, local, SpatialVerifier())

Two device kernels (csrc/asmk.hip) do the work: the aggregation of a batch of images into entries, and the scan of the inverted file
into a score panel that `pvs_topk_dev` ranks.  The inversion (a stable sort on words) and the integer weights are made on the host,
at build time only, in float64 as include/pvsim.h defines them; tests/asmk_numpy.py restates every value."""
from __future__ import annotations

import math

import numpy as np

from ._ffi import DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT

__all__ = ["ASMKIndex", "selectivity", "word_weights", "gammas", "random_projection"]

SCALE = 1023                       # sel[0], and the factor of gamma
IDF_SCALE = 64                     # wt = rint(64 ln(N / df))
MAX_ROWS = 8192                    # rows of one image (pvs_asmk_aggregate_dev)
MAX_MA = 8                         # words per query row (pvs_kmeans_topm_dev)
MAX_KEYS = 16384                   # rows x words of one query image (pvs_asmk_aggregate_ma_dev)
PANEL_BYTES = 64 << 20             # score panel of one query block
_KIND = "asmk_index"


# ------------------------------------------------------------------------------------------------ host arithmetic (float64)
def selectivity(bits: int, alpha: float = 3.0, tau: float = 0.0) -> np.ndarray:
    """sel int32 (bits + 1,): with u = 1 - 2 h / bits, rint(1023 u^alpha) where u > tau, 0 otherwise."""
    if bits not in (32, 64, 96, 128):
        raise ValueError(f"bits must be 32, 64, 96 or 128, got {bits!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError(f"alpha must be a positive number, got {alpha!r}")
    if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)) or not (0 <= tau < 1):
        raise ValueError(f"tau must lie in [0, 1), got {tau!r}")
    sel = np.zeros(bits + 1, np.int32)
    for h in range(bits + 1):
        u = 1.0 - 2.0 * h / bits
        if u > float(tau):
            sel[h] = int(np.rint(SCALE * u ** float(alpha)))
    return sel


def word_weights(df, n_images: int, idf: bool = True) -> np.ndarray:
    """df (K,) images per word -> wt int32 (K,): 0 where df = 0, else clip(rint(64 ln(N / df)), 1, 1023); 64 when idf is off."""
    df = np.asarray(df, np.int64)
    wt = np.zeros(len(df), np.int32)
    for w in np.flatnonzero(df):
        wt[w] = min(max(int(np.rint(IDF_SCALE * math.log(n_images / int(df[w])))), 1), 1023) if idf else IDF_SCALE
    return wt


def _weight_sums(ent_off, words, wt) -> np.ndarray:
    """int64 (n,): sum of 1023 wt[w] over each image's entries"""
    n = len(ent_off) - 1
    s = np.zeros(n, np.int64)
    if len(words):
        ok = (words >= 0) & (words < len(wt))
        np.add.at(s, np.repeat(np.arange(n), np.diff(ent_off))[ok], SCALE * wt[words[ok]].astype(np.int64))
    return s


def gammas(ent_off, words, wt) -> np.ndarray:
    """float32 (n,): 1 / sqrt(sum of 1023 wt[w] over the image's entries), 0 for an image without (weighted) entries."""
    s = _weight_sums(ent_off, words, wt)
    g = np.zeros(len(s), np.float32)
    nz = s > 0
    g[nz] = (1.0 / np.sqrt(s[nz].astype(np.float64))).astype(np.float32)
    return g


def random_projection(bits: int, dim: int, random_state=0) -> np.ndarray:
    """A seeded float32 (bits, dim) matrix with orthonormal rows (columns when bits > dim): Q of the QR of a normal draw, signs
    fixed by the diagonal of R."""
    rng = np.random.RandomState(random_state)
    m = max(bits, dim)
    q, r = np.linalg.qr(rng.standard_normal((m, m)))
    q = q * np.sign(np.where(np.diag(r) == 0, 1.0, np.diag(r)))[None, :]
    return np.ascontiguousarray(q[:bits, :dim], dtype=np.float32)


def _centroids(vocabulary) -> np.ndarray:
    c = getattr(vocabulary, "cluster_centers_", vocabulary)
    c = np.ascontiguousarray(c, dtype=np.float32)
    if c.ndim != 2 or not (1 <= c.shape[0] <= 65536) or not (1 <= c.shape[1] <= 128):
        raise ValueError(f"the vocabulary must be (K, D) centroids with 1 <= K <= 65536 and 1 <= D <= 128, got {c.shape}")
    return c


def _row_dtype(kind):
    if kind not in (DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT):
        raise ValueError(f"unknown descriptor kind {kind!r}")
    return np.uint8 if kind == DESC_U8_ROOTSIFT else np.float32


# ------------------------------------------------------------------------------------------------ device steps
def check_ma(ma, n_words: int, offsets=None) -> int:
    """`ma`, the words a query row is assigned to: an integer in 1..min(8, n_words).  With `offsets`, also the keys of the largest
    image: rows * ma <= 16384 (pvs_asmk_aggregate_ma_dev).  Raises before any device work."""
    if isinstance(ma, bool) or not isinstance(ma, (int, np.integer)) or not (1 <= ma <= min(MAX_MA, int(n_words))):
        raise ValueError(f"ma must be an integer in 1..{min(MAX_MA, int(n_words))}, got {ma!r}")
    ma = int(ma)
    if ma > 1 and offsets is not None:
        rows = int(np.diff(np.asarray(offsets, np.int64)).max(initial=0))
        if rows * ma > MAX_KEYS:
            raise NotImplementedError(f"a query of {rows} rows at ma = {ma} holds {rows * ma} keys, more than {MAX_KEYS}")
    return ma


def device_entries(ctx, cb, d_rows, offsets, kind, d_proj, bits, ma=1):
    """assign + aggregate + download + compact for the images whose rows lie at `d_rows` (device pointer) with host CSR `offsets`.
    -> (ent_off int64 (n + 1,), words int32 (E,), sigs uint32 (E, bits / 32)), image-major, words ascending inside an image.
    ma = 1: every row goes to its nearest word (pvs_kmeans_predict_dev + pvs_asmk_aggregate_dev); ma >= 2: to its ma nearest words
    (pvs_kmeans_topm_dev + pvs_asmk_aggregate_ma_dev), the multiple assignment of a QUERY's rows."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    ma = check_ma(ma, cb.K, offsets)
    n, total, W = len(offsets) - 1, int(offsets[-1]), bits // 32
    if n == 0 or total == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, W), np.uint32)
    slots = total * ma
    with ctx.scratch() as tmp:
        d_lab, d_word, d_sig, d_cnt, d_off = tmp(slots * 4), tmp(slots * 4), tmp(slots * 4 * W), tmp(n * 4), tmp.upload(offsets)
        if ma == 1:
            ctx.kmeans_predict_dev(cb, d_rows, kind, total, d_lab.ptr)
            ctx.asmk_aggregate_dev(cb, d_rows, kind, d_off.ptr, offsets, n, total, d_lab.ptr, d_proj, bits, d_word.ptr, d_sig.ptr, d_cnt.ptr)
        else:
            ctx.kmeans_topm_dev(cb, d_rows, kind, total, ma, d_lab.ptr)
            ctx.asmk_aggregate_ma_dev(cb, d_rows, kind, d_off.ptr, offsets, n, total, d_lab.ptr, ma, d_proj, bits, d_word.ptr, d_sig.ptr,
                                      d_cnt.ptr)
        counts = d_cnt.download((n,), np.int32).astype(np.int64)
        words = d_word.download((slots,), np.int32)
        sigs = d_sig.download((slots, W), np.uint32)
    ent_off = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=ent_off[1:])
    per = np.diff(offsets) * ma                                                              # slots of an image
    slot = np.arange(slots, dtype=np.int64) - np.repeat(offsets[:-1] * ma, per)             # position of a slot inside its image
    keep = slot < np.repeat(counts, per)
    return ent_off, np.ascontiguousarray(words[keep]), np.ascontiguousarray(sigs[keep])


def invert(ent_off, words, sigs, K):
    """image-major entries -> (word_off int64 (K + 1,), ent_img int32 (E,), ent_sig uint32 (E, W)) sorted by (word, image): a stable
    sort on words, as IVFCompactIndex sorts into lists."""
    img = np.repeat(np.arange(len(ent_off) - 1, dtype=np.int32), np.diff(ent_off))
    order = np.argsort(words, kind="stable")
    word_off = np.zeros(K + 1, np.int64)
    np.cumsum(np.bincount(words, minlength=K), out=word_off[1:])
    return word_off, np.ascontiguousarray(img[order]), np.ascontiguousarray(sigs[order])


# ------------------------------------------------------------------------------------------------ index
class ASMKIndex:
    """Paths + an inverted file of (image, signature) entries over visual words, resident on the device, searched by
    pvs_asmk_score_dev + pvs_topk_dev.

    Build one with `ASMKIndex.build` (a vocabulary you have) or `ASMKIndex.fit` (trains one).  The arrays are uploaded on first use.
    The index is immutable: `add` and `remove` name a rebuild, because document frequencies, and with them every weight and gamma,
    change with the set of images."""

    def __init__(self, paths, centroids, word_off, ent_img, ent_sig, gamma_db, wt, sel, bits, alpha=3.0, tau=0.0, idf=True,
                 projection=None, desc_kind=DESC_U8_ROOTSIFT, ctx=None, extractor=None):
        self._paths = list(paths)
        self.centroids = _centroids(centroids)
        K, D = self.centroids.shape
        self.bits = int(bits)
        if self.bits not in (32, 64, 96, 128):
            raise ValueError(f"bits must be 32, 64, 96 or 128, got {bits!r}")
        W = self.bits // 32
        self.word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        self.ent_img = np.ascontiguousarray(ent_img, dtype=np.int32)
        self.ent_sig = np.ascontiguousarray(ent_sig, dtype=np.uint32).reshape(-1, W)
        self.gamma_db = np.ascontiguousarray(gamma_db, dtype=np.float32)
        self.wt = np.ascontiguousarray(wt, dtype=np.int32)
        self.sel = np.ascontiguousarray(sel, dtype=np.int32)
        self.projection = None if projection is None else np.ascontiguousarray(projection, dtype=np.float32)
        _row_dtype(desc_kind)
        self.alpha, self.tau, self.idf, self.desc_kind = float(alpha), float(tau), bool(idf), int(desc_kind)
        N, E = len(self._paths), len(self.ent_img)
        if self.word_off.shape != (K + 1,) or self.word_off[0] != 0 or self.word_off[-1] != E or (np.diff(self.word_off) < 0).any():
            raise ValueError("word_off must be K + 1 non-decreasing offsets from 0 to the number of entries")
        if self.ent_sig.shape[0] != E or self.gamma_db.shape != (N,) or self.wt.shape != (K,) or self.sel.shape != (self.bits + 1,):
            raise ValueError("the arrays of the index do not fit together")
        if E and (self.ent_img.min() < 0 or self.ent_img.max() >= N):
            raise ValueError("an entry names an image outside the index")
        if self.projection is None and self.bits != D:
            raise ValueError(f"without a projection bits must equal D = {D}, got {self.bits}")
        if self.projection is not None and self.projection.shape != (self.bits, D):
            raise ValueError(f"the projection must be (bits, D) = {(self.bits, D)}, got {self.projection.shape}")
        self._ctx, self._extractor, self._dev = ctx, extractor, None

    # -------------------------------------------------------------------------------------------------- construction
    @classmethod
    def build(cls, local, vocabulary, bits: int = 128, alpha: float = 3.0, tau: float = 0.0, idf: bool = True, projection=None,
              random_state=0, desc_kind=DESC_U8_ROOTSIFT, extractor=None) -> "ASMKIndex":
        """Index the images of a `LocalFeatureIndex` against `vocabulary` ((K, D) centroids or a KMeansModel): assign, aggregate,
        download the counts, compact, invert on the host, make the weights, gamma and sel.  `projection`: None (needs bits == D),
        "random" (a seeded orthonormal matrix) or a (bits, D) array."""
        cent = _centroids(vocabulary)
        K, D = cent.shape
        if desc_kind != DESC_U8_ROOTSIFT:
            raise ValueError("the rows of a LocalFeatureIndex are uint8: only DESC_U8_ROOTSIFT reads them")
        if D != 128:
            raise ValueError(f"a LocalFeatureIndex holds rows of 128 values, the vocabulary has D = {D}")
        sel = selectivity(bits, alpha, tau)
        if isinstance(projection, str):
            if projection != "random":
                raise ValueError(f"projection must be None, 'random' or an array, got {projection!r}")
            projection = random_projection(bits, D, random_state)
        elif projection is not None:
            projection = np.ascontiguousarray(projection, dtype=np.float32)
            if projection.shape != (bits, D):
                raise ValueError(f"the projection must be (bits, D) = {(bits, D)}, got {projection.shape}")
        elif bits != D:
            raise ValueError(f"without a projection bits must equal D = {D}, got {bits}")
        if int(np.diff(local.offsets).max(initial=0)) > MAX_ROWS:
            raise NotImplementedError(f"an image of more than {MAX_ROWS} rows cannot be indexed")
        ctx = local.ctx
        cb = ctx.codebook(cent)
        try:
            with ctx.scratch() as tmp:
                d_proj = tmp.upload(projection).ptr if projection is not None else None
                ent_off, words, sigs = device_entries(ctx, cb, local.rows.ptr, local.offsets, desc_kind, d_proj, bits)
        finally:
            cb.close()
        N = len(local)
        word_off, ent_img, ent_sig = invert(ent_off, words, sigs, K)
        wt = word_weights(np.diff(word_off), N, idf)          # an image holds a word at most once: df = the length of the list
        return cls(local.paths, cent, word_off, ent_img, ent_sig, gammas(ent_off, words, wt), wt, sel, bits, alpha, tau, idf,
                   projection, desc_kind, ctx, extractor)

    @classmethod
    def fit(cls, local, n_words: int, train_rows: int | None = None, random_state=0, max_iter: int = 20, **build_kwargs) -> "ASMKIndex":
        """Train a vocabulary of `n_words` on a seeded sample of `train_rows` rows of `local` (default: all, at most 64 per word),
        then `build`.  The sample is materialised as RootSIFT rows on the device and clustered by learn.fit_kmeans."""
        from . import learn
        total = local.total_rows
        if isinstance(n_words, bool) or int(n_words) != n_words or not (1 <= n_words <= 65536):
            raise ValueError(f"n_words must be an integer in 1..65536, got {n_words!r}")
        if total < n_words:
            raise ValueError(f"{total} rows cannot train {n_words} words")
        want = min(total, 64 * int(n_words)) if train_rows is None else int(train_rows)
        if not (n_words <= want <= total):
            raise ValueError(f"train_rows must lie in n_words..{total}, got {train_rows!r}")
        kind = build_kwargs.get("desc_kind", DESC_U8_ROOTSIFT)
        ctx = local.ctx
        keep = np.zeros(total, np.uint8)
        keep[np.random.RandomState(random_state).permutation(total)[:want]] = 1
        with ctx.scratch() as tmp:                             # the sampled rows, in index order, gathered by the row compaction
            stage, out, d_keep, d_pos = tmp(want * 128), tmp(want * 128 * 4), tmp.upload(keep), tmp((total + 1) * 8)
            ctx.keep_positions_dev(d_keep.ptr, total, d_pos.ptr)
            ctx.compact_rows_dev(local.rows.ptr, total, 128, d_keep.ptr, d_pos.ptr, stage.ptr)
            ctx.materialise_dev(stage.ptr, kind, 128, want, out.ptr)
            ctx.sync()
            model = learn.fit_kmeans(learn.DeviceRows(ctx, want, 128, out), int(n_words), max_iter=max_iter, random_state=random_state)
        return cls.build(local, model, random_state=random_state, **build_kwargs)

    # -------------------------------------------------------------------------------------------------- access
    def __len__(self) -> int:
        return len(self._paths)

    @property
    def paths(self) -> list:
        return list(self._paths)

    @property
    def n_words(self) -> int:
        return self.centroids.shape[0]

    def list_sizes(self) -> np.ndarray:
        """entries per visual word, int64 (K,)"""
        return np.diff(self.word_off)

    @property
    def ctx(self):
        if self._ctx is None:
            from .engine import default_context
            self._ctx = default_context()
        return self._ctx

    @property
    def extractor(self):
        if self._extractor is None:
            from .features import KeypointRootSIFT
            self._extractor = KeypointRootSIFT(nfeatures=2000, ctx=self._ctx)
        return self._extractor

    def add(self, *args, **kwargs):
        raise NotImplementedError("an ASMKIndex is immutable: document frequencies, weights and gammas depend on the whole set of "
                                  "images -- rebuild it with ASMKIndex.build(local, vocabulary)")

    def remove(self, *args, **kwargs):
        raise NotImplementedError("an ASMKIndex is immutable: document frequencies, weights and gammas depend on the whole set of "
                                  "images -- rebuild it with ASMKIndex.build(local, vocabulary)")

    def _resident(self) -> dict:
        if self._dev is None:
            ctx = self.ctx
            dev = {"cb": ctx.codebook(self.centroids)}
            for name in ("word_off", "ent_img", "ent_sig", "gamma_db", "wt", "sel", "projection"):
                a = getattr(self, name)
                dev[name] = None if a is None else ctx.buffer(a.nbytes).upload(a) if a.nbytes else ctx.buffer(0)
            self._dev = dev
        return self._dev

    def close(self):
        if self._dev is not None:
            self._dev.pop("cb").close()
            for b in self._dev.values():
                if b is not None:
                    b.free()
            self._dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __repr__(self):
        return (f"ASMKIndex(images={len(self)}, words={self.n_words}, bits={self.bits}, entries={len(self.ent_img)}, "
                f"alpha={self.alpha}, tau={self.tau}, idf={self.idf})")

    # -------------------------------------------------------------------------------------------------- queries
    def query_entries(self, d_rows, offsets, ma=1):
        """entries of query images whose rows are on the device -> (ent_off, words, sigs); `ma`: words per row (1..min(8, n_words))"""
        ma = check_ma(ma, self.n_words, offsets)
        dev = self._resident()
        return device_entries(self.ctx, dev["cb"], d_rows, offsets, self.desc_kind,
                              dev["projection"].ptr if dev["projection"] is not None else None, self.bits, ma)

    def rank_entries(self, ent_off, words, sigs, k: int, slice_images: int = 0):
        """Rank the database for queries given as entries -> (idx int64 (nq, k), val float32 (nq, k)); slots that cannot be filled
        are idx = -1, val = -inf.  ValueError for a query whose weights could overflow the integer score."""
        ent_off = np.ascontiguousarray(ent_off, dtype=np.int64)
        words = np.ascontiguousarray(words, dtype=np.int32)
        W = self.bits // 32
        sigs = np.ascontiguousarray(sigs, dtype=np.uint32).reshape(-1, W)
        nq, N = len(ent_off) - 1, len(self)
        if isinstance(k, bool) or int(k) != k or k < 1:
            raise ValueError(f"k must be a positive integer, got {k!r}")
        k = int(k)
        sums = _weight_sums(ent_off, words, self.wt)
        if nq and int(sums.max()) >= 1 << 32:
            raise ValueError(f"query {int(sums.argmax())} holds entries whose weights sum to 2^32 or more: the integer score could "
                             "overflow (4104 entries are always safe)")
        idx, val = np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, np.float32)
        if nq == 0 or N == 0:
            return idx, val
        kk = min(k, N)
        gq = gammas(ent_off, words, self.wt)
        ctx, dev = self.ctx, self._resident()
        qb = int(max(1, min(nq, PANEL_BYTES // (4 * N))))
        with ctx.scratch() as tmp:
            d_word, d_sig, d_gq = tmp.upload(words), tmp.upload(sigs), tmp.upload(gq)
            d_panel, d_idx, d_val = tmp(qb * N * 4), tmp(nq * kk * 8), tmp(nq * kk * 4)
            for q0 in range(0, nq, qb):                     # whole rows of the panel: each block's ranking is final
                qn = min(qb, nq - q0)
                ctx.asmk_score_dev(qn, ent_off[q0:q0 + qn + 1], d_word.ptr, d_sig.ptr, self.bits, self.n_words, dev["word_off"].ptr,
                                   dev["ent_img"].ptr, dev["ent_sig"].ptr, N, dev["wt"].ptr, dev["sel"].ptr, d_gq.ptr + q0 * 4,
                                   dev["gamma_db"].ptr, d_panel.ptr, N, slice_images)
                ctx.topk_dev(d_panel.ptr, qn, N, N, kk, 0, 0, d_idx.ptr + q0 * kk * 8, d_val.ptr + q0 * kk * 4)
            idx[:, :kk] = d_idx.download((nq, kk), np.int64)
            val[:, :kk] = d_val.download((nq, kk), np.float32)
        return idx, val

    def rank_rows(self, rows_list, k: int, ma=1):
        """Rank the database for queries given as host descriptor rows (one (n, D) array per query, uint8 for DESC_U8_ROOTSIFT).
        `ma`: the nearest words every query row is assigned to (the paper uses 5); the database stays single assignment."""
        ma = check_ma(ma, self.n_words)
        D = self.centroids.shape[1]
        dt = _row_dtype(self.desc_kind)
        rows_list = [np.ascontiguousarray(r, dtype=dt).reshape(-1, D) for r in rows_list]
        if any(len(r) > MAX_ROWS for r in rows_list):
            raise NotImplementedError(f"a query of more than {MAX_ROWS} rows is not supported")
        off = np.zeros(len(rows_list) + 1, np.int64)
        np.cumsum([len(r) for r in rows_list], out=off[1:])
        total = int(off[-1])
        check_ma(ma, self.n_words, off)
        with self.ctx.scratch() as tmp:
            d_rows = tmp.upload(np.concatenate(rows_list) if total else np.zeros((0, D), dt))
            ent = self.query_entries(d_rows.ptr, off, ma)
        return self.rank_entries(*ent, k)

    def rank_images(self, images, k: int, ma=1):
        """Rank the database for query images (arrays or paths), extracted with the index's extractor; `ma` as in rank_rows."""
        from .verify import LocalFeatureIndex
        ma = check_ma(ma, self.n_words)
        if self.desc_kind != DESC_U8_ROOTSIFT:
            raise ValueError("images are extracted as uint8 rows: the index must read DESC_U8_ROOTSIFT")
        q = LocalFeatureIndex.from_images(list(images), self.extractor, ctx=self.ctx)
        try:
            if int(np.diff(q.offsets).max(initial=0)) > MAX_ROWS:
                raise NotImplementedError(f"a query of more than {MAX_ROWS} rows is not supported")
            ent = self.query_entries(q.rows.ptr, q.offsets, ma)
        finally:
            q.close()
        return self.rank_entries(*ent, k)

    def retrieve(self, query_image, k: int = 100, ma=1) -> list:
        """-> [(path, score)] best first: the `hits` that eval.rerank_spatial takes.  `ma`: words per query row (rank_rows)."""
        idx, val = self.rank_images([query_image], k, ma)
        return [(self._paths[int(i)], float(v)) for i, v in zip(idx[0], val[0]) if i >= 0]

    # -------------------------------------------------------------------------------------------------- persistence
    def save(self, path: str) -> None:
        """One plain .npz of arrays (numpy.load(allow_pickle=False)), kind = "asmk_index"."""
        ints = all(isinstance(p, (int, np.integer)) and not isinstance(p, bool) for p in self._paths)
        arrays = dict(kind=_KIND, paths=np.array(self._paths, dtype=np.int64 if ints else np.str_), centroids=self.centroids,
                      word_off=self.word_off, ent_img=self.ent_img, ent_sig=self.ent_sig, gamma_db=self.gamma_db, wt=self.wt, sel=self.sel,
                      params=np.array([self.bits, self.alpha, self.tau, float(self.idf), self.desc_kind], np.float64))
        if self.projection is not None:
            arrays["projection"] = self.projection
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path: str, ctx=None, extractor=None) -> "ASMKIndex":
        with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
            if "kind" not in z.files or str(z["kind"]) != _KIND:
                raise ValueError(f"{path}: not an ASMK index file")
            p = z["params"]
            paths = [int(v) for v in z["paths"]] if z["paths"].dtype.kind in "iu" else [str(v) for v in z["paths"]]
            return cls(paths, z["centroids"], z["word_off"], z["ent_img"], z["ent_sig"], z["gamma_db"], z["wt"], z["sel"], int(p[0]),
                       float(p[1]), float(p[2]), bool(p[3]), z["projection"] if "projection" in z.files else None, int(p[4]), ctx,
                       extractor)
