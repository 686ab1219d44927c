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
into a score panel that `pvs_topk_dev` ranks.  The inversion (a stable sort on words) is made on the host by default and on the
device with `build(..., on_device=True)` (csrc/asmk_update.hip); the integer weights are made on the host, in float64 as
include/pvsim.h defines them; tests/asmk_numpy.py restates every value.

An index whose weights belong to the vocabulary and not to the indexed set is FROZEN (`build(..., weights=wt)` or `freeze()`), and
a frozen index takes new images and gives up old ones without a rebuild:

    index.freeze()
    local.add(new); index.add(new)                               # `new`: a LocalFeatureIndex of the new images
    local.remove(paths); index.remove(paths)

Query expansion on the entries (`ASMKExpansion`, csrc/asmk_expand.hip; tests/asmk_expand_numpy.py restates it):
the best results of a first ranking refine the signatures of the query's words and add the words they agree on, on the device:

    hits = index.retrieve(query_image, k=100, expand=ASMKExpansion(n=10, min_support=2))"""
from __future__ import annotations

import math

import numpy as np

from ._ffi import DESC_F32, DESC_F32_ROOTSIFT, DESC_U8_ROOTSIFT

__all__ = ["ASMKIndex", "ASMKExpansion", "selectivity", "word_weights", "gammas", "random_projection"]

SCALE = 1023                       # sel[0], and the factor of gamma
IDF_SCALE = 64                     # wt = rint(64 ln(N / df))
MAX_ROWS = 8192                    # rows of one image (pvs_asmk_aggregate_dev)
MAX_MA = 8                         # words per query row (pvs_kmeans_topm_dev)
MAX_KEYS = 16384                   # rows x words of one query image (pvs_asmk_aggregate_ma_dev)
PANEL_BYTES = 64 << 20             # score panel of one query block
MAX_MEMBERS = 32                   # members of one query (pvs_asmk_expand_dev)
MAX_QUERY_VOTE = 65535
EXPAND_BYTES = 256 << 20           # expanded entries of one query block
PAD_BYTE = 0x7F                    # fills the unwritten tail of a row of expanded words: 0x7F7F7F7F is no word, the score skips it
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


def _gammas_of_sums(s) -> np.ndarray:
    g = np.zeros(len(s), np.float32)
    nz = s > 0
    g[nz] = (1.0 / np.sqrt(s[nz].astype(np.float64))).astype(np.float32)
    return g


def gammas(ent_off, words, wt) -> np.ndarray:
    """float32 (n,): 1 / sqrt(sum of 1023 wt[w] over the image's entries), 0 for an image without (weighted) entries."""
    return _gammas_of_sums(_weight_sums(ent_off, words, wt))


def check_weights(weights, K: int) -> np.ndarray:
    """`weights=` of build: an integer array (K,) with every value in 0..1023 -> int32 (K,); anything else is a ValueError"""
    w = np.asarray(weights)
    if w.dtype.kind not in "iu" or w.shape != (int(K),):
        raise ValueError(f"weights must be an integer array of shape ({int(K)},), got {w.dtype} {w.shape}")
    if w.size and (int(w.min()) < 0 or int(w.max()) > SCALE):
        raise ValueError(f"every weight must lie in 0..{SCALE}, got {int(w.min())}..{int(w.max())}")
    return np.ascontiguousarray(w, dtype=np.int32)


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


def _check_k(k) -> int:
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"k must be a positive integer, got {k!r}")
    return int(k)


def _check_rows(offsets, query: bool = False) -> None:
    """no image of the CSR `offsets` holds more than 8192 rows (pvs_asmk_aggregate_dev)"""
    if int(np.diff(offsets).max(initial=0)) > MAX_ROWS:
        raise NotImplementedError(f"a query of more than {MAX_ROWS} rows is not supported" if query else
                                  f"an image of more than {MAX_ROWS} rows cannot be indexed")


def _free_file(bufs) -> None:
    """the three device buffers of a file set (ASMKIndex._file_buffers)"""
    for name in ("word_off", "ent_img", "ent_sig"):
        bufs[name].free()


def _proj_ptr(buf):
    """the device pointer of an optional projection buffer"""
    return None if buf is None else buf.ptr


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


def device_invert(ctx, tmp, cb, d_rows, offsets, kind, d_proj, bits, img_base=0, tile_entries=0) -> dict:
    """assign + aggregate + pvs_asmk_invert_dev for a batch whose rows lie at `d_rows`: nothing but K + 1 offsets comes back.
    -> dict(n, total, word_off (host int64 (K + 1,)), d_word_off, d_img, d_sig (arrays of `total` slots, word_off[K] of them
    defined), sums(d_wt) -> host int64 (n,) weight sums).  Every buffer belongs to the scratch block `tmp`; tmp.keep() takes one."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, total, W, K = len(offsets) - 1, int(offsets[-1]), bits // 32, cb.K
    d_lab, d_word, d_sig, d_cnt, d_off = tmp(total * 4), tmp(total * 4), tmp(total * 4 * W), tmp(n * 4), tmp.upload(offsets)
    d_woff, d_img, d_osig = tmp((K + 1) * 8), tmp(total * 4), tmp(total * 4 * W)
    if total:
        ctx.kmeans_predict_dev(cb, d_rows, kind, total, d_lab.ptr)
        ctx.asmk_aggregate_dev(cb, d_rows, kind, d_off.ptr, offsets, n, total, d_lab.ptr, d_proj, bits, d_word.ptr, d_sig.ptr, d_cnt.ptr)
    ctx.asmk_invert_dev(K, bits, d_off.ptr, offsets, n, d_cnt.ptr, d_word.ptr, d_sig.ptr, img_base, d_woff.ptr, d_img.ptr, d_osig.ptr,
                        tile_entries)

    def sums(d_wt):
        if n == 0:
            return np.zeros(0, np.int64)
        d_sums = tmp(n * 8)
        ctx.asmk_weight_sums_dev(K, d_off.ptr, offsets, n, d_cnt.ptr, d_word.ptr, d_wt, d_sums.ptr)
        return d_sums.download((n,), np.int64)

    return dict(n=n, total=total, word_off=d_woff.download((K + 1,), np.int64), d_word_off=d_woff, d_img=d_img, d_sig=d_osig, sums=sums)


# ------------------------------------------------------------------------------------------------ query expansion
def _check_int(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not (lo <= v <= hi):
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


class ASMKExpansion:
    """How `ASMKIndex.rank_*`, `retrieve` and `expand_verified` re-query (Tolias and Jegou, Pattern Recognition
    2014): the first `n` results of the previous ranking are the members; the signature of every query word becomes the majority
    vote of the query's own signature (`query_vote` votes) and the signatures the members store for that word within Hamming
    distance `h_max` of the query's (default bits // 4); a word the query lacks is added when at least `min_support` members hold it
    (0: no word is added).  `scheme` "flat" gives every member the vote 1 (`query_vote` defaults to 2), "linear" gives the member at
    rank j the vote n - j (`query_vote` defaults to n).  `passes` > 1 repeats this from the lists of the expanded query; every pass
    expands the original entries."""

    def __init__(self, n: int = 10, h_max=None, min_support: int = 2, query_vote=None, scheme: str = "flat", passes: int = 1):
        self.n = _check_int("n", n, 1, MAX_MEMBERS)
        self.h_max = None if h_max is None else _check_int("h_max", h_max, 0, 128)
        self.min_support = _check_int("min_support", min_support, 0, MAX_MEMBERS + 1)
        if scheme not in ("flat", "linear"):
            raise ValueError(f"scheme must be 'flat' or 'linear', got {scheme!r}")
        self.scheme = scheme
        default = 2 if scheme == "flat" else self.n
        self.query_vote = default if query_vote is None else _check_int("query_vote", query_vote, 0, MAX_QUERY_VOTE)
        if isinstance(passes, (bool, np.bool_)) or not isinstance(passes, (int, np.integer)) or passes < 1:
            raise ValueError(f"passes must be an integer >= 1, got {passes!r}")
        self.passes = int(passes)

    def resolve_h_max(self, bits: int) -> int:
        """h_max for signatures of `bits` bits: the default is bits // 4; a value above bits is a ValueError"""
        if self.h_max is None:
            return int(bits) // 4
        if self.h_max > bits:
            raise ValueError(f"h_max = {self.h_max} exceeds the {bits} bits of a signature")
        return self.h_max

    def members_of(self, idx):
        """ranked lists idx (nq, >= 0 slots; -1 where a slot is not filled) -> (members int32 (nq, n), votes int32 (nq, n)): the
        filled slots among the first n, ids ascending with -1 behind them, every vote beside its member"""
        idx = np.asarray(idx, np.int64)
        if idx.ndim != 2:
            raise ValueError("the ranked lists must be a 2-d array")
        nq, n = idx.shape[0], self.n
        lists = np.full((nq, n), -1, np.int64)
        lists[:, :min(n, idx.shape[1])] = idx[:, :n]
        rank_vote = np.ones(n, np.int64) if self.scheme == "flat" else n - np.arange(n, dtype=np.int64)
        votes = np.broadcast_to(rank_vote, (nq, n)).copy()
        for q in range(nq):
            ids = lists[q][lists[q] >= 0]
            if len(np.unique(ids)) != len(ids):
                raise ValueError(f"query {q} names a member twice")
        key = np.where(lists >= 0, lists, np.iinfo(np.int64).max)
        order = np.argsort(key, axis=1, kind="stable")
        members = np.take_along_axis(lists, order, axis=1)
        votes = np.where(members >= 0, np.take_along_axis(votes, order, axis=1), 0)
        return np.ascontiguousarray(members, dtype=np.int32), np.ascontiguousarray(votes, dtype=np.int32)

    def __repr__(self):
        return (f"ASMKExpansion(n={self.n}, h_max={self.h_max}, min_support={self.min_support}, query_vote={self.query_vote}, "
                f"scheme={self.scheme!r}, passes={self.passes})")


def check_expanded_sums(sums, expansion) -> None:
    """the weight sums of expanded queries (int64, from the device): ValueError where one reaches 2^32"""
    sums = np.asarray(sums, np.int64)
    if sums.size and int(sums.max()) >= 1 << 32:
        raise ValueError(f"the expanded query {int(sums.argmax())} holds entries whose weights sum to 2^32 or more: the integer score "
                         f"could overflow -- raise min_support (now {expansion.min_support}) or lower n (now {expansion.n}), so that "
                         "fewer words are added")


def _check_members(members, votes, nq, N):
    """members / votes as the device takes them: int32 (nq, R), ids strictly ascending in [0, N) then -1, votes in 1..1023"""
    members, votes = np.ascontiguousarray(members, dtype=np.int32), np.ascontiguousarray(votes, dtype=np.int32)
    if members.ndim != 2 or members.shape != votes.shape or members.shape[0] != nq or members.shape[1] > MAX_MEMBERS:
        raise ValueError(f"members and votes must both be (nq, R) = ({nq}, R <= {MAX_MEMBERS}), got {members.shape} and {votes.shape}")
    live = members >= 0
    if (live[:, 1:] & ~live[:, :-1]).any() or (members < -1).any():
        raise ValueError("the members of a query come first, -1 padding behind them")
    if (members >= N).any():
        raise ValueError(f"a member id is not below the {N} images of the index")
    if (live[:, 1:] & (members[:, 1:] <= members[:, :-1])).any():
        raise ValueError("the members of a query must ascend strictly")
    if ((votes[live] < 1) | (votes[live] > SCALE)).any():
        raise ValueError(f"every vote must lie in 1..{SCALE}")
    return members, votes


_NOT_FROZEN = ("an ASMKIndex whose weights come from the indexed set is immutable: document frequencies, weights and gammas depend on "
               "the whole set of images -- rebuild it with ASMKIndex.build(local, vocabulary), or hold the weights fixed with "
               "freeze() or build(..., weights=) and update it in place")


# ------------------------------------------------------------------------------------------------ index
class ASMKIndex:
    """Paths + an inverted file of (image, signature) entries over visual words, resident on the device, searched by
    pvs_asmk_score_dev + pvs_topk_dev.

    Build one with `ASMKIndex.build` (a vocabulary you have) or `ASMKIndex.fit` (trains one).  The arrays are uploaded on first use.
    An index whose weights derive from its own images is immutable: `add` and `remove` name a rebuild, because document
    frequencies, and with them every weight and gamma, change with the set of images.  A FROZEN index (`freeze()`, or
    `build(..., weights=wt)`) holds its weights fixed; `add`, `remove` and `del index[path]` then move data on the device, and the
    result equals `build(<the surviving images in surviving order>, vocabulary, weights=index.wt, ...)` array for array.  After an
    update or a device build `ent_img`, `ent_sig` and `gamma_db` are downloaded when first read; `word_off` is always on the host."""

    def __init__(self, paths, centroids, word_off, ent_img, ent_sig, gamma_db, wt, sel, bits, alpha=3.0, tau=0.0, idf=True,
                 projection=None, desc_kind=DESC_U8_ROOTSIFT, ctx=None, extractor=None, frozen=False):
        self._paths = list(paths)
        self.centroids = _centroids(centroids)
        K, D = self.centroids.shape
        self.bits = int(bits)
        if self.bits not in (32, 64, 96, 128):
            raise ValueError(f"bits must be 32, 64, 96 or 128, got {bits!r}")
        W = self.bits // 32
        self.word_off = np.ascontiguousarray(word_off, dtype=np.int64)
        on_device = ent_img is None and ent_sig is None       # _build_on_device: the two arrays are resident, and come from the kernels
        self.ent_img = None if on_device else np.ascontiguousarray(ent_img, dtype=np.int32)
        self.ent_sig = None if on_device else np.ascontiguousarray(ent_sig, dtype=np.uint32).reshape(-1, W)
        self.gamma_db = np.ascontiguousarray(gamma_db, dtype=np.float32)
        self.wt = np.ascontiguousarray(wt, dtype=np.int32)
        self.sel = np.ascontiguousarray(sel, dtype=np.int32)
        self.projection = None if projection is None else np.ascontiguousarray(projection, dtype=np.float32)
        _row_dtype(desc_kind)
        self.alpha, self.tau, self.idf, self.desc_kind = float(alpha), float(tau), bool(idf), int(desc_kind)
        N = len(self._paths)
        E = len(self.ent_img) if not on_device else int(self.word_off[-1]) if self.word_off.size else 0
        if self.word_off.shape != (K + 1,) or self.word_off[0] != 0 or self.word_off[-1] != E or (np.diff(self.word_off) < 0).any():
            raise ValueError("word_off must be K + 1 non-decreasing offsets from 0 to the number of entries")
        if (not on_device and self.ent_sig.shape[0] != E) or self.gamma_db.shape != (N,) or self.wt.shape != (K,) or self.sel.shape != (self.bits + 1,):
            raise ValueError("the arrays of the index do not fit together")
        if E and not on_device and (self.ent_img.min() < 0 or self.ent_img.max() >= N):
            raise ValueError("an entry names an image outside the index")
        if self.projection is None and self.bits != D:
            raise ValueError(f"without a projection bits must equal D = {D}, got {self.bits}")
        if self.projection is not None and self.projection.shape != (self.bits, D):
            raise ValueError(f"the projection must be (bits, D) = {(self.bits, D)}, got {self.projection.shape}")
        self._ctx, self._extractor, self._dev = ctx, extractor, None
        self._frozen, self._spare, self._cap_e, self._cap_n = bool(frozen), None, 0, 0

    # the three arrays that an update leaves on the device: host copies made when first read
    def _host(self, name, shape, dtype):
        a = self.__dict__.get("_h_" + name)
        if a is None:
            buf = self._dev[name]
            a = buf.download(shape, dtype) if int(np.prod(shape)) else np.zeros(shape, dtype)
            self.__dict__["_h_" + name] = a
        return a

    @property
    def ent_img(self) -> np.ndarray:
        return self._host("ent_img", (int(self.word_off[-1]),), np.int32)

    @ent_img.setter
    def ent_img(self, a):
        self.__dict__["_h_ent_img"] = a

    @property
    def ent_sig(self) -> np.ndarray:
        return self._host("ent_sig", (int(self.word_off[-1]), self.bits // 32), np.uint32)

    @ent_sig.setter
    def ent_sig(self, a):
        self.__dict__["_h_ent_sig"] = a

    @property
    def gamma_db(self) -> np.ndarray:
        return self._host("gamma_db", (len(self._paths),), np.float32)

    @gamma_db.setter
    def gamma_db(self, a):
        self.__dict__["_h_gamma_db"] = a

    def _stale(self):
        """the device holds the truth: forget the host copies"""
        self.ent_img = self.ent_sig = self.gamma_db = None

    # -------------------------------------------------------------------------------------------------- construction
    @classmethod
    def build(cls, local, vocabulary, bits: int = 128, alpha: float = 3.0, tau: float = 0.0, idf: bool = True, projection=None,
              random_state=0, desc_kind=DESC_U8_ROOTSIFT, extractor=None, weights=None, on_device: bool = False) -> "ASMKIndex":
        """Index the images of a `LocalFeatureIndex` against `vocabulary` ((K, D) centroids or a KMeansModel): assign, aggregate,
        download the counts, compact, invert on the host, make the weights, gamma and sel.  `projection`: None (needs bits == D),
        "random" (a seeded orthonormal matrix) or a (bits, D) array.

        `weights`: int32 (K,) with every value in 0..1023, e.g. the `wt` of an index over a training corpus.  The index uses them as
        they are (`idf` is recorded but derives nothing) and is frozen: it can be updated in place.
        `on_device=True` inverts on the device as well: only the K + 1 offsets and one weight sum per image come back, and the
        inverted file never leaves the device.  Both routes give the same arrays byte for byte."""
        cent = _centroids(vocabulary)
        K, D = cent.shape
        if weights is not None:
            weights = check_weights(weights, K)
        if not isinstance(on_device, (bool, np.bool_)):
            raise ValueError(f"on_device must be a bool, got {on_device!r}")
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
        _check_rows(local.offsets)
        ctx = local.ctx
        if on_device:
            return cls._build_on_device(local, cent, sel, bits, alpha, tau, idf, projection, desc_kind, ctx, extractor, weights)
        cb = ctx.codebook(cent)
        try:
            with ctx.scratch() as tmp:
                d_proj = tmp.upload(projection).ptr if projection is not None else None
                ent_off, words, sigs = device_entries(ctx, cb, local.rows.ptr, local.offsets, desc_kind, d_proj, bits)
        finally:
            cb.close()
        N = len(local)
        word_off, ent_img, ent_sig = invert(ent_off, words, sigs, K)
        # an image holds a word at most once: df = the length of the list
        wt = word_weights(np.diff(word_off), N, idf) if weights is None else weights
        return cls(local.paths, cent, word_off, ent_img, ent_sig, gammas(ent_off, words, wt), wt, sel, bits, alpha, tau, idf,
                   projection, desc_kind, ctx, extractor, weights is not None)

    @classmethod
    def _build_on_device(cls, local, cent, sel, bits, alpha, tau, idf, projection, desc_kind, ctx, extractor, weights):
        N = len(local)
        cb = ctx.codebook(cent)
        dev = {"cb": cb}
        try:
            with ctx.scratch() as tmp:
                d_proj = tmp.upload(projection).ptr if projection is not None else None
                got = device_invert(ctx, tmp, cb, local.rows.ptr, local.offsets, desc_kind, d_proj, bits)
                word_off = got["word_off"]
                wt = word_weights(np.diff(word_off), N, idf) if weights is None else weights
                dev["wt"] = ctx.buffer(wt.nbytes).upload(wt)
                gamma = _gammas_of_sums(got["sums"](dev["wt"].ptr))
                dev["word_off"], dev["ent_img"], dev["ent_sig"] = tmp.keep(got["d_word_off"]), tmp.keep(got["d_img"]), tmp.keep(got["d_sig"])
            dev["gamma_db"] = ctx.buffer(gamma.nbytes).upload(gamma) if N else ctx.buffer(0)
            dev["sel"] = ctx.buffer(sel.nbytes).upload(sel)
            dev["projection"] = None if projection is None else ctx.buffer(projection.nbytes).upload(projection)
        except Exception:
            for b in dev.values():
                if b is not None:
                    (b.close if b is cb else b.free)()
            raise
        self = cls(local.paths, cent, word_off, None, None, gamma, wt, sel, bits, alpha, tau, idf, projection, desc_kind, ctx, extractor,
                   weights is not None)
        self._dev, self._cap_e, self._cap_n = dev, got["total"], N
        return self

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

    # -------------------------------------------------------------------------------------------------- frozen weights and updates
    @property
    def frozen(self) -> bool:
        """True when `wt` is a property of the vocabulary, not of the indexed set: the index can be updated in place."""
        return self._frozen

    def freeze(self, unseen_weight: int = 0) -> "ASMKIndex":
        """Declare the weights fixed from now on, so that `add` and `remove` work; returns self.

        `unseen_weight`, an integer in 0..1023, is given to the words whose weight is 0 at this moment: the words no image held.
        The default 0 changes no bit of any score or ranking.  A non-zero value changes gamma(Q) of the queries that hold such
        words (their scores against every image scale down), and lets images added later match on them; with 0 such words stay
        silent in later adds: their entries are stored, but weigh nothing."""
        if isinstance(unseen_weight, (bool, np.bool_)) or not isinstance(unseen_weight, (int, np.integer)) or not (0 <= unseen_weight <= SCALE):
            raise ValueError(f"unseen_weight must be an integer in 0..{SCALE}, got {unseen_weight!r}")
        if unseen_weight and (self.wt == 0).any():
            self.wt = np.where(self.wt == 0, np.int32(unseen_weight), self.wt).astype(np.int32)
            if self._dev is not None:
                self._dev["wt"].upload(self.wt)
        self._frozen = True
        return self

    def _new_batch(self, source, rows_list):
        """the arguments of add -> (paths, offsets, LocalFeatureIndex or None, host rows or None), checked, before any device work"""
        if hasattr(source, "offsets") and hasattr(source, "rows") and rows_list is None:
            if self.desc_kind != DESC_U8_ROOTSIFT:
                raise ValueError("the rows of a LocalFeatureIndex are uint8: only DESC_U8_ROOTSIFT reads them")
            paths, off, rows = list(source.paths), np.ascontiguousarray(source.offsets, dtype=np.int64), None
        else:
            if rows_list is None:
                raise ValueError("add takes a LocalFeatureIndex, or paths and one array of rows per path")
            paths, source = list(source), None
            D, dt = self.centroids.shape[1], _row_dtype(self.desc_kind)
            rows_list = [np.ascontiguousarray(r, dtype=dt).reshape(-1, D) for r in rows_list]
            if len(rows_list) != len(paths):
                raise ValueError(f"{len(paths)} paths but {len(rows_list)} arrays of rows")
            off = np.zeros(len(paths) + 1, np.int64)
            np.cumsum([len(r) for r in rows_list], out=off[1:])
            rows = np.concatenate(rows_list) if int(off[-1]) else np.zeros((0, D), dt)
        have = set(self._paths)
        for p in paths:
            if p in have:
                raise ValueError(f"{p!r} is already in the index (or named twice)")
            have.add(p)
        _check_rows(off)
        return paths, off, source, rows

    def _file_buffers(self, cap):
        ctx, W = self.ctx, self.bits // 32
        return {"word_off": ctx.buffer((self.n_words + 1) * 8), "ent_img": ctx.buffer(cap * 4), "ent_sig": ctx.buffer(cap * 4 * W), "cap": cap}

    def _other(self, need):
        """the buffers an out-of-place update writes: the spare set, replaced by a larger one when `need` entries do not fit"""
        sp, self._spare = self._spare, None
        if sp is None or sp["cap"] < need:
            if sp is not None:
                _free_file(sp)
            sp = self._file_buffers(max(need, 2 * self._cap_e if need > self._cap_e else self._cap_e, 1))
        return sp

    def _swap(self, out):
        """`out` becomes the file, the file becomes the spare"""
        dev = self._dev
        self._spare = {"word_off": dev["word_off"], "ent_img": dev["ent_img"], "ent_sig": dev["ent_sig"], "cap": self._cap_e}
        dev["word_off"], dev["ent_img"], dev["ent_sig"], self._cap_e = out["word_off"], out["ent_img"], out["ent_sig"], out["cap"]

    def _ensure_capacity(self):
        """after the first upload the buffers hold exactly what the host arrays held"""
        if self._cap_e == 0 and self._cap_n == 0:
            self._cap_e, self._cap_n = int(self.word_off[-1]), len(self._paths)

    def reserve(self, entries: int) -> "ASMKIndex":
        """Make room for `entries` entries in the inverted file, so that adds up to that size allocate nothing; returns self."""
        if isinstance(entries, (bool, np.bool_)) or not isinstance(entries, (int, np.integer)) or entries < 0:
            raise ValueError(f"entries must be a non-negative integer, got {entries!r}")
        if entries >= 1 << 31:
            raise NotImplementedError("list maintenance serves fewer than 2^31 entries")
        dev = self._resident()
        E = int(self.word_off[-1])
        if entries > self._cap_e:
            ctx, W = self.ctx, self.bits // 32
            out = self._file_buffers(int(entries))
            ctx.copy_dev(out["word_off"].ptr, dev["word_off"].ptr, (self.n_words + 1) * 8)
            ctx.copy_dev(out["ent_img"].ptr, dev["ent_img"].ptr, E * 4)
            ctx.copy_dev(out["ent_sig"].ptr, dev["ent_sig"].ptr, E * 4 * W)
            self._swap(out)
            sp, self._spare = self._spare, None
            _free_file(sp)
        return self

    def add(self, source=None, rows_list=None, *args, **kwargs):
        """Append images: `add(local)` with a LocalFeatureIndex reads its resident rows in place and takes its paths;
        `add(paths, rows_list)` takes one host array of rows per path (uint8 for DESC_U8_ROOTSIFT).  The new images get the ids
        N, N + 1, ...; a path the index already holds is a ValueError before anything changes; an empty batch is a no-op.
        NotImplementedError on an index that is not frozen (see `freeze`)."""
        if not self._frozen:
            raise NotImplementedError(_NOT_FROZEN)
        if args or kwargs:
            raise TypeError("add takes a LocalFeatureIndex, or paths and rows_list")
        paths, off, local, rows = self._new_batch(source, rows_list)
        n = len(paths)
        if n == 0:
            return self
        ctx, dev = self.ctx, self._resident()
        K, N, E = self.n_words, len(self._paths), int(self.word_off[-1])
        with ctx.scratch() as tmp:
            d_rows = local.rows.ptr if local is not None else tmp.upload(rows).ptr
            d_proj = _proj_ptr(dev["projection"])
            got = device_invert(ctx, tmp, dev["cb"], d_rows, off, self.desc_kind, d_proj, self.bits, img_base=N)
            new_off = got["word_off"]
            b = int(new_off[-1])
            if E + b >= 1 << 31:
                raise NotImplementedError("list maintenance serves fewer than 2^31 entries")
            gamma_new = _gammas_of_sums(got["sums"](dev["wt"].ptr))
            out = self._other(E + b)
            try:
                ctx.asmk_insert_dev(K, self.bits, dev["word_off"].ptr, self.word_off, dev["ent_img"].ptr, dev["ent_sig"].ptr,
                                    got["d_word_off"].ptr, new_off, got["d_img"].ptr, got["d_sig"].ptr, out["word_off"].ptr,
                                    out["ent_img"].ptr, out["ent_sig"].ptr)
            except Exception:
                self._spare = out
                raise
            if N + n > self._cap_n:
                cap = max(N + n, 2 * self._cap_n)
                g = ctx.buffer(cap * 4)
                ctx.copy_dev(g.ptr, dev["gamma_db"].ptr, N * 4)
                dev["gamma_db"].free()
                dev["gamma_db"], self._cap_n = g, cap
            dev["gamma_db"].upload(gamma_new, N * 4)
            ctx.sync()                                        # the batch's buffers go back to the pool with the block
        self._swap(out)
        self.word_off = self.word_off + new_off
        self._paths = self._paths + paths
        self._stale()
        return self

    def remove(self, paths=None, *args, **kwargs):
        """Drop the named images; the survivors keep their order and are renumbered 0 .. N' - 1.  An unknown path is a KeyError, a
        path named twice a ValueError, both before anything changes; an empty list is a no-op.  NotImplementedError on an index
        that is not frozen (see `freeze`)."""
        if not self._frozen:
            raise NotImplementedError(_NOT_FROZEN)
        if args or kwargs:
            raise TypeError("remove takes a list of paths")
        paths = list(paths if paths is not None else [])
        where = {p: i for i, p in enumerate(self._paths)}
        gone = []
        for p in paths:
            if p not in where:
                raise KeyError(p)
            gone.append(where[p])
        if len(set(gone)) != len(gone):
            raise ValueError("a path is named twice")
        if not gone:
            return self
        ctx, dev = self.ctx, self._resident()
        K, N, E = self.n_words, len(self._paths), int(self.word_off[-1])
        removed = np.sort(np.array(gone, np.int64))
        out = self._other(E)
        with ctx.scratch() as tmp:
            d_removed, d_keep, d_pos = tmp.upload(removed), tmp(N), tmp((N + 1) * 8)
            ctx.keep_mask_dev(d_removed.ptr, len(removed), N, d_keep.ptr)
            ctx.keep_positions_dev(d_keep.ptr, N, d_pos.ptr)
            try:
                ctx.asmk_remove_dev(K, self.bits, N, dev["word_off"].ptr, self.word_off, dev["ent_img"].ptr, dev["ent_sig"].ptr, d_keep.ptr,
                                    d_pos.ptr, out["word_off"].ptr, out["ent_img"].ptr, out["ent_sig"].ptr)
            except Exception:
                self._spare = out
                raise
            ctx.compact_rows_dev(dev["gamma_db"].ptr, N, 4, d_keep.ptr, d_pos.ptr, dev["gamma_db"].ptr, first=int(removed[0]))
            word_off = out["word_off"].download((K + 1,), np.int64)
        self._swap(out)
        self.word_off = word_off
        dead = set(gone)
        self._paths = [p for i, p in enumerate(self._paths) if i not in dead]
        self._stale()
        return self

    def __delitem__(self, path):
        self.remove([path])

    def _resident(self) -> dict:
        if self._dev is None:
            ctx = self.ctx
            dev = {"cb": ctx.codebook(self.centroids)}
            for name in ("word_off", "ent_img", "ent_sig", "gamma_db", "wt", "sel", "projection"):
                a = getattr(self, name)
                dev[name] = None if a is None else ctx.buffer(a.nbytes).upload(a) if a.nbytes else ctx.buffer(0)
            self._dev = dev
        self._ensure_capacity()
        return self._dev

    def close(self):
        if self._dev is not None:
            _ = self.ent_img, self.ent_sig, self.gamma_db    # what only the device holds comes to the host first
            self._dev.pop("cb").close()
            for b in self._dev.values():
                if b is not None:
                    b.free()
            self._dev = None
            self._cap_e = self._cap_n = 0
        if self._spare is not None:
            _free_file(self._spare)
            self._spare = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __repr__(self):
        return (f"ASMKIndex(images={len(self)}, words={self.n_words}, bits={self.bits}, entries={int(self.word_off[-1])}, "
                f"alpha={self.alpha}, tau={self.tau}, idf={self.idf})")

    # -------------------------------------------------------------------------------------------------- queries
    def query_entries(self, d_rows, offsets, ma=1):
        """entries of query images whose rows are on the device -> (ent_off, words, sigs); `ma`: words per row (1..min(8, n_words))"""
        ma = check_ma(ma, self.n_words, offsets)
        dev = self._resident()
        return device_entries(self.ctx, dev["cb"], d_rows, offsets, self.desc_kind, _proj_ptr(dev["projection"]), self.bits, ma)

    def _query_arrays(self, ent_off, words, sigs):
        ent_off = np.ascontiguousarray(ent_off, dtype=np.int64)
        words = np.ascontiguousarray(words, dtype=np.int32)
        sigs = np.ascontiguousarray(sigs, dtype=np.uint32).reshape(-1, self.bits // 32)
        return ent_off, words, sigs

    def _rank_dev(self, tmp, d_word, d_sig, h_off, gq, k, slice_images=0):
        """score + top-k for queries whose entries lie on the device (host offsets `h_off`, host gammas `gq`) -> (idx (nq, k), val
        (nq, k)) on the host, slots that cannot be filled idx = -1, val = -inf.  N > 0 and nq > 0."""
        ctx, dev, nq, N = self.ctx, self._resident(), len(h_off) - 1, len(self)
        idx, val = np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, np.float32)
        kk = min(k, N)
        qb = int(max(1, min(nq, PANEL_BYTES // (4 * N))))
        d_gq = tmp.upload(gq)
        d_panel, d_idx, d_val = tmp(qb * N * 4), tmp(nq * kk * 8), tmp(nq * kk * 4)
        for q0 in range(0, nq, qb):                     # whole rows of the panel: each block's ranking is final
            qn = min(qb, nq - q0)
            ctx.asmk_score_dev(qn, h_off[q0:q0 + qn + 1], d_word.ptr, d_sig.ptr, self.bits, self.n_words, dev["word_off"].ptr,
                               dev["ent_img"].ptr, dev["ent_sig"].ptr, N, dev["wt"].ptr, dev["sel"].ptr, d_gq.ptr + q0 * 4,
                               dev["gamma_db"].ptr, d_panel.ptr, N, slice_images)
            ctx.topk_dev(d_panel.ptr, qn, N, N, kk, 0, 0, d_idx.ptr + q0 * kk * 8, d_val.ptr + q0 * kk * 4)
        idx[:, :kk] = d_idx.download((nq, kk), np.int64)
        val[:, :kk] = d_val.download((nq, kk), np.float32)
        return idx, val

    def _query_sums(self, ent_off, words):
        sums = _weight_sums(ent_off, words, self.wt)
        if len(sums) and int(sums.max()) >= 1 << 32:
            raise ValueError(f"query {int(sums.argmax())} holds entries whose weights sum to 2^32 or more: the integer score could "
                             "overflow (4104 entries are always safe)")
        return sums

    def rank_entries(self, ent_off, words, sigs, k: int, slice_images: int = 0, expand=None):
        """Rank the database for queries given as entries -> (idx int64 (nq, k), val float32 (nq, k)); slots that cannot be filled
        are idx = -1, val = -inf.  ValueError for a query whose weights could overflow the integer score.

        `expand`: None, or an `ASMKExpansion`: rank to depth n, take the filled slots of each list as members (ids ascending for
        the device, every vote beside its member), expand the entries (pvs_asmk_expand_dev), rank the expanded queries to depth k.
        The expanded entries stay on the device between the expansion and the score; only counts, weight sums and ranked lists
        come to the host.  One host synchronisation per pass is inherent: the score takes its entry offsets and gamma(Q) from the
        host, and gamma(Q), like the 2^32 guard, needs the weight sum the expansion found."""
        ent_off, words, sigs = self._query_arrays(ent_off, words, sigs)
        nq, N = len(ent_off) - 1, len(self)
        k = _check_k(k)
        if expand is not None:
            return self._rank_expanded(ent_off, words, sigs, k, expand, slice_images)
        sums = self._query_sums(ent_off, words)
        if nq == 0 or N == 0:
            return np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, np.float32)
        with self.ctx.scratch() as tmp:
            d_word, d_sig = tmp.upload(words), tmp.upload(sigs)
            return self._rank_dev(tmp, d_word, d_sig, ent_off, _gammas_of_sums(sums), k, slice_images)

    # -------------------------------------------------------------------------------------------------- query expansion
    def _expand_cap(self, ent_off, R):
        """entries one expanded query can hold: its own and at most 8192 per member, never more than the words there are"""
        longest = int(np.diff(ent_off).max(initial=0))
        return max(1, min(self.n_words, longest + int(R) * MAX_ROWS))

    def _expand_dev(self, tmp, d_word, d_sig, ent_off, members, votes, expansion, out=None):
        """one pvs_asmk_expand_dev call and one download of counts and sums.  -> dict(d_word, d_sig: rows of `cap` slots per query
        over a fill that the score skips; cap; off: the host offsets q * cap of the rows; counts int64 (nq,); sums int64 (nq,))"""
        if not isinstance(expansion, ASMKExpansion):
            raise TypeError("expand must be a pvsim.ASMKExpansion")
        ctx, dev, nq, W = self.ctx, self._resident(), len(ent_off) - 1, self.bits // 32
        members, votes = _check_members(members, votes, nq, len(self))
        R, h_max = members.shape[1], expansion.resolve_h_max(self.bits)
        cap = self._expand_cap(ent_off, R) if out is None else out["cap"]
        if out is None:
            out = dict(d_word=tmp(nq * cap * 4), d_sig=tmp(nq * cap * 4 * W), cap=cap)
        d_cs = tmp(nq * 12)                                    # sums int64 (nq,), then counts int32 (nq,)
        d_mem, d_vote = tmp.upload(members), tmp.upload(votes)
        out["d_word"].fill_bytes(PAD_BYTE)
        ctx.asmk_expand_dev(nq, ent_off, d_word.ptr, d_sig.ptr, self.bits, self.n_words, dev["word_off"].ptr, dev["ent_img"].ptr,
                            dev["ent_sig"].ptr, len(self), R, d_mem.ptr, d_vote.ptr, expansion.query_vote, h_max,
                            expansion.min_support, dev["wt"].ptr, cap, out["d_word"].ptr, out["d_sig"].ptr, d_cs.ptr + nq * 8, d_cs.ptr)
        raw = d_cs.download((nq * 12,), np.uint8)
        sums, counts = raw[:nq * 8].view(np.int64).copy(), raw[nq * 8:].view(np.int32).astype(np.int64)
        if int(counts.max(initial=0)) > cap:
            raise RuntimeError(f"an expanded query holds {int(counts.max())} entries, more than the {cap} that can occur")
        check_expanded_sums(sums, expansion)
        return dict(out, off=np.arange(nq + 1, dtype=np.int64) * cap, counts=counts, sums=sums)

    def expand_entries(self, ent_off, words, sigs, members, votes, expansion):
        """The entries of queries, expanded by the entries the index stores for their members -> (ent_off', words', sigs') on the
        host, in the layout of `query_entries`.  `members` int32 (nq, R): per query its image ids strictly ascending, -1 behind
        them; `votes` int32 (nq, R) in 1..1023 (`ASMKExpansion.members_of` makes both from ranked lists).  One device call and
        one download of counts and sums, then the entries themselves.  ValueError when the weights of an expanded query sum to
        2^32 or more."""
        ent_off, words, sigs = self._query_arrays(ent_off, words, sigs)
        nq, W = len(ent_off) - 1, self.bits // 32
        if nq == 0:
            return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, W), np.uint32)
        with self.ctx.scratch() as tmp:
            x = self._expand_dev(tmp, tmp.upload(words), tmp.upload(sigs), ent_off, members, votes, expansion)
            cap, counts = x["cap"], x["counts"]
            keep = np.arange(cap)[None, :] < counts[:, None]
            out_words = x["d_word"].download((nq, cap), np.int32)[keep]
            out_sigs = x["d_sig"].download((nq, cap, W), np.uint32)[keep]
        off = np.zeros(nq + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        return off, np.ascontiguousarray(out_words), np.ascontiguousarray(out_sigs)

    def _rank_expanded(self, ent_off, words, sigs, k, expansion, slice_images=0, members=None, votes=None):
        """rank_entries with an ASMKExpansion.  `members` / `votes`: the members of the first pass where they do not come from a
        ranking of the plain query (expand_verified)."""
        if not isinstance(expansion, ASMKExpansion):
            raise TypeError("expand must be a pvsim.ASMKExpansion")
        nq, N, W = len(ent_off) - 1, len(self), self.bits // 32
        sums = self._query_sums(ent_off, words)
        if nq == 0 or N == 0:
            return np.full((nq, k), -1, np.int64), np.full((nq, k), -np.inf, np.float32)
        expansion.resolve_h_max(self.bits)
        cap = self._expand_cap(ent_off, expansion.n)
        qb = int(max(1, EXPAND_BYTES // (cap * 4 * (W + 1))))
        if nq > qb:                                            # blocks of queries whose expanded entries fit the budget
            parts = []
            for q0 in range(0, nq, qb):
                q1, lo, hi = min(q0 + qb, nq), int(ent_off[q0]), int(ent_off[min(q0 + qb, nq)])
                parts.append(self._rank_expanded(ent_off[q0:q1 + 1] - lo, words[lo:hi], sigs[lo:hi], k, expansion, slice_images,
                                                 None if members is None else members[q0:q1], None if votes is None else votes[q0:q1]))
            return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        n = expansion.n
        with self.ctx.scratch() as tmp:
            d_word, d_sig = tmp.upload(words), tmp.upload(sigs)
            if members is None:
                with self.ctx.scratch() as first:
                    idx, _ = self._rank_dev(first, d_word, d_sig, ent_off, _gammas_of_sums(sums), n, slice_images)
                members, votes = expansion.members_of(idx)
            out = dict(d_word=tmp(nq * cap * 4), d_sig=tmp(nq * cap * 4 * W), cap=cap)
            for p in range(expansion.passes):
                last = p == expansion.passes - 1
                with self.ctx.scratch() as step:
                    x = self._expand_dev(step, d_word, d_sig, ent_off, members, votes, expansion, out)
                    idx, val = self._rank_dev(step, x["d_word"], x["d_sig"], x["off"], _gammas_of_sums(x["sums"]), k if last else n,
                                              slice_images)
                if not last:
                    members, votes = expansion.members_of(idx)
        return idx, val

    def expand_verified(self, query_image, ranked, k: int = 100, expand=None, min_inliers: int = 4, ma=1) -> list:
        """Query expansion over spatially verified results, the analogue of `eval.expand_verified` for this index: `ranked` is what
        `eval.rerank_spatial` returned, [(path, score, inliers)]; the members are its first `expand.n` paths with at least
        `min_inliers` inliers (the default expansion is ASMKExpansion()), in that order for the votes of the "linear" scheme; the k
        best images for the expanded query come back as [(path, score)].  With no verified path there is nothing to expand with:
        the first k of `ranked`, without the inlier counts.  KeyError for a path the index does not hold."""
        expand = ASMKExpansion() if expand is None else expand
        if not isinstance(expand, ASMKExpansion):
            raise TypeError("expand must be a pvsim.ASMKExpansion")
        if isinstance(min_inliers, bool) or int(min_inliers) != min_inliers or min_inliers < 0:
            raise ValueError(f"min_inliers must be a non-negative integer, got {min_inliers!r}")
        k = _check_k(k)
        ma = check_ma(ma, self.n_words)
        ranked = list(ranked)
        verified = [path for path, _, inliers in ranked if inliers >= min_inliers][:expand.n]
        if not verified or len(self) == 0:
            return [(path, score) for path, score, _ in ranked[:int(k)]]
        where = {p: i for i, p in enumerate(self._paths)}
        for path in verified:
            if path not in where:
                raise KeyError(path)
        members, votes = expand.members_of(np.array([[where[p] for p in verified]], np.int64))
        ent_off, words, sigs = self._query_arrays(*self._image_entries([query_image], ma))
        idx, val = self._rank_expanded(ent_off, words, sigs, int(k), expand, members=members, votes=votes)
        return [(self._paths[int(i)], float(v)) for i, v in zip(idx[0], val[0]) if i >= 0]

    def rank_rows(self, rows_list, k: int, ma=1, expand=None):
        """Rank the database for queries given as host descriptor rows (one (n, D) array per query, uint8 for DESC_U8_ROOTSIFT).
        `ma`: the nearest words every query row is assigned to (the paper uses 5); the database stays single assignment.
        `expand`: None or an `ASMKExpansion` (rank_entries)."""
        ma = check_ma(ma, self.n_words)
        D = self.centroids.shape[1]
        dt = _row_dtype(self.desc_kind)
        rows_list = [np.ascontiguousarray(r, dtype=dt).reshape(-1, D) for r in rows_list]
        off = np.zeros(len(rows_list) + 1, np.int64)
        np.cumsum([len(r) for r in rows_list], out=off[1:])
        _check_rows(off, query=True)
        total = int(off[-1])
        check_ma(ma, self.n_words, off)
        with self.ctx.scratch() as tmp:
            d_rows = tmp.upload(np.concatenate(rows_list) if total else np.zeros((0, D), dt))
            ent = self.query_entries(d_rows.ptr, off, ma)
        return self.rank_entries(*ent, k, expand=expand)

    def _image_entries(self, images, ma):
        """the entries of query images (arrays or paths), extracted with the index's extractor -> (ent_off, words, sigs)"""
        from .verify import LocalFeatureIndex
        if self.desc_kind != DESC_U8_ROOTSIFT:
            raise ValueError("images are extracted as uint8 rows: the index must read DESC_U8_ROOTSIFT")
        q = LocalFeatureIndex.from_images(list(images), self.extractor, ctx=self.ctx)
        try:
            _check_rows(q.offsets, query=True)
            return self.query_entries(q.rows.ptr, q.offsets, ma)
        finally:
            q.close()

    def rank_images(self, images, k: int, ma=1, expand=None):
        """Rank the database for query images (arrays or paths), extracted with the index's extractor; `ma` and `expand` as in
        rank_rows."""
        ma = check_ma(ma, self.n_words)
        return self.rank_entries(*self._image_entries(images, ma), k, expand=expand)

    def retrieve(self, query_image, k: int = 100, ma=1, expand=None) -> list:
        """-> [(path, score)] best first: the `hits` that eval.rerank_spatial takes.  `ma`: words per query row (rank_rows);
        `expand`: None or an `ASMKExpansion` (rank_entries)."""
        idx, val = self.rank_images([query_image], k, ma, expand)
        return [(self._paths[int(i)], float(v)) for i, v in zip(idx[0], val[0]) if i >= 0]

    # -------------------------------------------------------------------------------------------------- persistence
    def save(self, path: str) -> None:
        """One plain .npz of arrays (numpy.load(allow_pickle=False)), kind = "asmk_index"."""
        ints = all(isinstance(p, (int, np.integer)) and not isinstance(p, bool) for p in self._paths)
        arrays = dict(kind=_KIND, paths=np.array(self._paths, dtype=np.int64 if ints else np.str_), centroids=self.centroids,
                      word_off=self.word_off, ent_img=self.ent_img, ent_sig=self.ent_sig, gamma_db=self.gamma_db, wt=self.wt, sel=self.sel,
                      params=np.array([self.bits, self.alpha, self.tau, float(self.idf), self.desc_kind], np.float64),
                      frozen=np.array(self._frozen))
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
                       extractor, bool(z["frozen"]) if "frozen" in z.files else False)
